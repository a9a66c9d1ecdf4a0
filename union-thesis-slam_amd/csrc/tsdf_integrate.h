// tsdf_integrate.h -- the host code of an integrate call that the dense grid and the voxel hash
// share (included by tsdf_dense.hip and tsdf_hash.hip only; each keeps its kernels, this code
// launches none): the loop of the fused path and the front end of the deferred per-frame calls.
#pragma once
#include "tsdf_host.h"

#ifndef TSDF_HOST_TIME  // (the hash's diagnostic host timers: defined ahead of this header there)
#define TSDF_HOST_TIME(slot) ((void)0)
#endif

namespace tsdf {

// The fused path: the launches of the schedule in tsdf_pipeline.h, the buffer sets rotated by
// rot.  Before launch L the host prepares the batch of its prep stage in that batch's set and
// slot.  The policy P is the handle's part, passed by reference, all members inline: tex (the
// batches carry texels), gi, gc, cw (Base::fill_stage), finish (its own Stage fields and what
// must precede the launch), launch, integrated (after a launch with an integrate, its staging
// slot still held) and released (the slot handed back).
template <class P>
int run_fused(Base& B, P& pol, int n_frames, const void* depth, int dk, const void* color, int H, int W,
              const double* K, const double* Tinv, const double* ow, int flags, int rot) {
    const int nb = pipe_batches(n_frames, B.batch);
    static const Batch kNone{};
    Batch bts[kSets];
    TexelScope tex_scope(B, pol.tex);
    for (int L = -2; L < nb; ++L) {
        const PipeStep st = pipe_step(L, nb, B.batch, n_frames, rot);
        if (st.p.on) {
            B.use_set(st.p.set);
            TSDF_HOST_TIME(2);
            TSDF_TRY(B.prepare_batch(&bts[st.p.at], depth, dk, color, TSDF_COLOR_RGB8, H, W, K, Tinv, ow, 1.0,
                                     flags, st.p.f0, st.p.n, st.p.slot));
        }
        const Batch& bi = st.i.on ? bts[st.i.at] : kNone;
        const Batch& bc = st.c.on ? bts[st.c.at] : kNone;
        const Batch& bp = st.p.on ? bts[st.p.at] : kNone;
        Stage sg{};
        unsigned grid = 0;
        TSDF_TRY(B.fill_stage(&sg, st, pol.gi, pol.gc, pol.cw, H, W, &grid));
        TSDF_TRY(pol.finish(st, sg));
        hipEvent_t e0 = nullptr;
        if (st.i.on) TSDF_TRY(B.prof.begin(B.stream, &e0));
        TSDF_HOST_TIME(3);
        pol.launch(grid, bi, bc, bp, sg);
        TSDF_HIP(hipGetLastError());
        if (!st.i.on) continue;
        TSDF_TRY(B.prof.end(B.stream, e0));
        B.frames += bi.n;
        TSDF_TRY(pol.integrated(bi, sg));
        TSDF_TRY(B.end_batch(flags, st.i.slot));  // batch L's frames: last read by this launch
        TSDF_TRY(pol.released());
    }
    return TSDF_OK;
}

// The TSDF_DEFER branch of the per-frame integrate: the frame joins the handle's deferred batch,
// which runs (flush(wait); wait = false: the full batch) when it is full or when a frame of
// another kind arrives.  before_push: the handle's own step ahead of a push that may reallocate.
template <class Flush, class Hook>
int integrate_deferred(Base& B, const void* depth, int dk, const void* color, int ck, int H, int W,
                       const double* K, const double* T, double ow, int flags, Flush flush, Hook before_push) {
    if (flags & TSDF_DEVICE_PTRS) return set_error(TSDF_E_ARG, "TSDF_DEFER takes host frames only");
    if (B.dfr.n > 0 && !B.defer_same(dk, ck, H, W, K)) TSDF_TRY(flush(true));
    TSDF_TRY(before_push());
    int r = B.defer_push(depth, dk, color, ck, H, W, K, T, ow);
    if (r == Base::kDeferFlush) {  // the batch's frames went as u16 and this one cannot
        TSDF_TRY(flush(true));
        r = B.defer_push(depth, dk, color, ck, H, W, K, T, ow);
    }
    TSDF_TRY(r);
    if (B.dfr.n == B.defer_frames) TSDF_TRY(flush(false));
    return TSDF_OK;
}

}  // namespace tsdf
