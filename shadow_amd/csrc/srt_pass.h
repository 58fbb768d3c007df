/*
 * srt_pass.h -- host-side plumbing shared by the launchers of the row passes (routes.hip,
 * linkload.hip, envelope.hip, splitload.hip): the goto-out HIP check, the persistent grid's size
 * and the per-launch scratch with its stat words. Each launcher keeps its own launch, LDS size,
 * scratch layout and event bracket.
 */
#ifndef SRT_PASS_H
#define SRT_PASS_H

#include "srt_device.h"

/* a HIP call inside a function with `int rc` and an `out:` label */
#define SRT_PASS_TRY(x)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            srt_set_error("HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); \
            rc = SRT_E_DEVICE;                                                                 \
            goto out;                                                                          \
        }                                                                                      \
    } while (0)

/* the most scratch one launch takes: the grid shrinks to stay under it */
#define SRT_PASS_SCRATCH_BYTES ((size_t)8 << 30)

/* the persistent grid of a pass over nrows rows: the workgroups the LDS lets a CU hold (two unless
 * lds passes 76 KiB or the pass asks for one), fewer where grid * per_block would pass
 * SRT_PASS_SCRATCH_BYTES, at most one a row */
static inline int srt_pass_grid(size_t lds, size_t per_block, int nrows, bool one_per_cu) {
    const int cus = srt_cu_count();
    int grid = one_per_cu || lds > 76 * 1024 ? cus : 2 * cus;
    if (per_block && (size_t)grid * per_block > SRT_PASS_SCRATCH_BYTES)
        grid = (int)(SRT_PASS_SCRATCH_BYTES / per_block) > 0
                   ? (int)(SRT_PASS_SCRATCH_BYTES / per_block) : 1;
    return nrows < grid ? nrows : grid;
}

/* the scratch block and the zeroed stat words of one launch, both from srt_scratch_pool. open,
 * launch, finish: finish must follow every open that returned SRT_OK */
struct srt_pass_scratch {
    const char* pass = NULL; /* the pass's name in messages ("route pass", "link load") */
    hipStream_t st = NULL;
    char* ws = NULL;    /* ws_bytes of scratch (NULL where ws_bytes is 0) */
    void* dstat = NULL; /* stat_bytes, zeroed */
    size_t stat_bytes = 0;

    int open(const char* name, hipStream_t stream, size_t ws_bytes, size_t nstat) {
        int rc = SRT_OK;
        pass = name;
        st = stream;
        stat_bytes = nstat;
        if (ws_bytes && srt_malloc_async((void**)&ws, ws_bytes, st) != hipSuccess) {
            (void)hipGetLastError();
            ws = NULL;
            srt_set_error("%s: scratch of %zu MiB failed", pass, ws_bytes >> 20);
            return SRT_E_NOMEM;
        }
        SRT_PASS_TRY(srt_malloc_async((void**)&dstat, stat_bytes, st));
        SRT_PASS_TRY(hipMemsetAsync(dstat, 0, stat_bytes, st));
        return SRT_OK;
    out:
        (void)finish(rc, NULL);
        return rc;
    }

    /* rc: the launch's outcome so far. Copies the stat words into hstat where rc is SRT_OK, frees
     * both blocks and returns after the stream */
    int finish(int rc, void* hstat) {
        if (!rc && hstat)
            SRT_PASS_TRY(hipMemcpyAsync(hstat, dstat, stat_bytes, hipMemcpyDeviceToHost, st));
    out:
        if (ws) (void)hipFreeAsync(ws, st);
        if (dstat) (void)hipFreeAsync(dstat, st);
        ws = NULL;
        dstat = NULL;
        if (hipStreamSynchronize(st) != hipSuccess && !rc) {
            srt_set_error("%s: the kernel failed (%s)", pass, hipGetErrorString(hipGetLastError()));
            rc = SRT_E_DEVICE;
        }
        return rc;
    }
};

#endif
