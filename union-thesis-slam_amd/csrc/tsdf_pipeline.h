// tsdf_pipeline.h -- the launch schedule of one integrate call in plain integers (no HIP: the
// CPU test, tools/check_pipeline.cpp, compiles this header alone).  DESIGN.md §6 states it.
//
// A call runs nb batches of nbat frames (the last may be short).  The fused path issues launches
// L = -2 .. nb-1: launch L integrates batch L, culls L+1 and preps L+2.  Batch j has place
// j % kSets in the call's Batch array, buffer set (j + rot) % kSets from its prep to its integrate
// (rot: 0 for the dense grid, carried from call to call by the hash) and, for host frames,
// staging slot j % kSlots from the host's copy before launch j-2 until launch j ends.  The
// in-line path runs a batch's three stages back to back in set 0: same frames, same slots.
#pragma once

namespace tsdf {

constexpr int kSets = 3;
constexpr int kSlots = 4;

struct PipeStage {
    bool on;               // the launch has this stage (else the other fields are 0)
    int j, at, set, slot;  // its batch; the batch's place, buffer set and staging slot
    int f0, n;             // the batch's frames [f0, f0 + n) of the call
};
struct PipeStep { PipeStage i, c, p; };  // integrate, cull, prep

inline int pipe_batches(int n_frames, int nbat) { return (n_frames + nbat - 1) / nbat; }

inline PipeStage pipe_stage(int j, int nb, int nbat, int n_frames, int rot) {
    if (j < 0 || j >= nb) return {};
    const int f0 = j * nbat;
    return {true, j, j % kSets, (j + rot) % kSets, j % kSlots, f0, n_frames - f0 < nbat ? n_frames - f0 : nbat};
}

// launch L (-2 .. nb-1) of a call of nb batches
inline PipeStep pipe_step(int L, int nb, int nbat, int n_frames, int rot) {
    return {pipe_stage(L, nb, nbat, n_frames, rot), pipe_stage(L + 1, nb, nbat, n_frames, rot),
            pipe_stage(L + 2, nb, nbat, n_frames, rot)};
}

inline int pipe_rot_after(int rot, int nb) { return (rot + nb) % kSets; }  // the next call's rot

}  // namespace tsdf
