// check_pipeline.cpp -- the integrate's launch schedule (csrc/tsdf_pipeline.h), checked on the CPU
// over calls of 1..9 batches of 1, 2, 8 and 32 frames and every rotation of the buffer sets.
//   g++ -std=c++17 -fsanitize=address,undefined -I union-thesis-slam_amd/csrc tools/check_pipeline.cpp
// Prints one line per property, "pipeline <name> checked <n> bad <n>"; exit status 1 if any is bad.
#include <cstdio>

#include "tsdf_pipeline.h"

using namespace tsdf;

namespace {

enum { kLaunches, kOnce, kSameSet, kDistinct, kSlots_, kFrames, kRot, kDense, kInline, kNProps };
const char* const kNames[kNProps] = {"launches", "once", "same_set", "distinct", "slots",
                                     "frames",   "rot",  "dense",    "inline"};
long long g_checked[kNProps], g_bad[kNProps];

void check(int prop, bool ok) {
    ++g_checked[prop];
    if (!ok) ++g_bad[prop];
}

constexpr int kMaxNb = 9;

void check_call(int nbat, int nb, int n_frames, int rot) {
    check(kFrames, pipe_batches(n_frames, nbat) == nb);
    // where each batch meets each stage: the launch, and the set / place / slot / frames it is given
    int count[3][kMaxNb] = {}, at_launch[3][kMaxNb], set[3][kMaxNb], slot[3][kMaxNb], f0[3][kMaxNb], n[3][kMaxNb];
    int launches = 0;
    for (int L = -5; L < nb + 3; ++L) {  // (a wider range than the loop's: nothing may happen outside it)
        const PipeStep st = pipe_step(L, nb, nbat, n_frames, rot);
        const PipeStage* sg[3] = {&st.i, &st.c, &st.p};
        const bool any = st.i.on || st.c.on || st.p.on;
        launches += any;
        check(kLaunches, any == (L >= -2 && L < nb));
        for (int k = 0; k < 3; ++k) {
            if (!sg[k]->on) continue;
            const int j = sg[k]->j;
            check(kOnce, j == L + k && j >= 0 && j < nb);
            if (j < 0 || j >= nb) continue;
            ++count[k][j];
            at_launch[k][j] = L;
            set[k][j] = sg[k]->set;
            slot[k][j] = sg[k]->slot;
            f0[k][j] = sg[k]->f0;
            n[k][j] = sg[k]->n;
            check(kDistinct, sg[k]->at >= 0 && sg[k]->at < kSets && sg[k]->set >= 0 && sg[k]->set < kSets &&
                                 sg[k]->slot >= 0 && sg[k]->slot < kSlots);
            // the batches of one launch: pairwise distinct sets and places in the Batch array
            for (int m = 0; m < k; ++m)
                if (sg[m]->on) check(kDistinct, sg[m]->set != sg[k]->set && sg[m]->at != sg[k]->at);
        }
    }
    check(kLaunches, launches == nb + 2);
    int sum = 0;
    for (int j = 0; j < nb; ++j) {
        // prepped in launch j-2, culled in j-1, integrated in j, once each
        bool once = true;
        for (int k = 0; k < 3; ++k) once = once && count[k][j] == 1 && at_launch[k][j] == j - k;
        check(kOnce, once);
        if (!once) continue;
        check(kSameSet, set[0][j] == set[1][j] && set[1][j] == set[2][j]);
        check(kSameSet, slot[0][j] == slot[1][j] && slot[1][j] == slot[2][j] && f0[0][j] == f0[2][j] &&
                            f0[1][j] == f0[2][j] && n[0][j] == n[2][j] && n[1][j] == n[2][j]);
        check(kFrames, f0[2][j] == j * nbat && n[2][j] >= 1 && n[2][j] <= nbat && (n[2][j] == nbat || j == nb - 1));
        sum += n[2][j];
        if (rot == 0) check(kDense, set[2][j] == j % kSets);
        // the slot the host fills before launch L = j-2: not that of the batches L-1, L, L+1 (still
        // to be read, or being read by the launch in flight), but that of L-2, whose integrate was issued
        for (int d = 1; d <= 3; ++d)
            if (j - d >= 0) check(kSlots_, slot[2][j] != slot[0][j - d]);
        if (j - 4 >= 0) check(kSlots_, slot[2][j] == slot[0][j - 4]);
        // the in-line walk: the same frames, slot j % kSlots
        const PipeStage b = pipe_stage(j, nb, nbat, n_frames, 0);
        check(kInline, b.on && b.f0 == f0[2][j] && b.n == n[2][j] && b.slot == j % kSlots);
    }
    check(kFrames, sum == n_frames);
    check(kRot, pipe_rot_after(rot, nb) == (rot + nb) % kSets && pipe_rot_after(rot, nb) >= 0 &&
                    pipe_rot_after(rot, nb) < kSets);
}

}  // namespace

int main() {
    const int nbats[] = {1, 2, 8, 32};
    for (int nbat : nbats)
        for (int nb = 1; nb <= kMaxNb; ++nb)
            for (int n_frames = (nb - 1) * nbat + 1; n_frames <= nb * nbat; ++n_frames)
                for (int rot = 0; rot < kSets; ++rot) check_call(nbat, nb, n_frames, rot);
    long long bad = 0;
    for (int p = 0; p < kNProps; ++p) {
        std::printf("pipeline %s checked %lld bad %lld\n", kNames[p], g_checked[p], g_bad[p]);
        bad += g_bad[p];
    }
    return bad ? 1 : 0;
}
