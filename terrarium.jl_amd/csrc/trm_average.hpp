// trm_average.hpp -- time averages of fields (trm_average_*, AveragedTimeInterval): the accumulation on the device.
//
// An accumulator is a `double` array laid out like the device buffer of its field ([Nh][Nzp] for 3-D fields, [Nh] for 2-D ones).
// Every step taken by a stepping entry point adds to it, per launch, the partial sum
//     P = sum_k (double)dt_k * (double)x_k          (x_k: the field after step k of the launch; P starts at 0.0)
// with the product and the sum rounded separately (the library builds with -ffp-contract=off).  Two paths form P:
//   - the resident multi-step program (k_column_accum, trm_column.hpp): every step adds dt * x into register partials of the
//     requested fields, which leave once per launch (acc = acc + P);
//   - everything else: one k_accumulate launch after every step launch, reading the field from memory (one step per launch, so
//     P is the single term dt * x).
#pragma once
#include "trm_device.hpp"

namespace trm {

// The fields the fused path accumulates, one slot each: the 3-D fields are held per lane (5 partials), the 2-D ones by lane
// k = slot - ACC_S of the column (one partial per lane, fed from the top lane by a shuffle).
enum {
    ACC_U = 0, ACC_SAT, ACC_T, ACC_LIQ, ACC_PSI,                  // 3-D
    ACC_S, ACC_WT,                                                // 2-D, SoilModel and LandModel
    ACC_TS, ACC_GHF, ACC_SWU, ACC_LWU, ACC_RNET, ACC_HS, ACC_HL, ACC_EVAP, ACC_INFIL, ACC_RUNOFF,   // 2-D, LandModel
    ACC_SLOTS
};
constexpr int ACC_3D = ACC_S;   // slots below are 3-D

// Fourth kernel argument of k_column_accum: where the partials of the requested slots go (dst[s] += P) and the step length the
// launch weights with (the caller's double dt, not the context precision's).  `mask`: bit per requested slot (wave-uniform).
struct AccumArgs {
    double* dst[ACC_SLOTS];
    double dt;
    unsigned mask;
};

// ---- k_accumulate: one launch for every open accumulator (trm_launch_average.hip) ----------------------------------------
// entry j of a batch: sum[e] = sum[e] + w * (double)src[e] over the elements of the device buffer whose level is a real cell
// (e % pitch < nz), src of the context precision -- or, for a partial the fused path left in a scratch buffer (src_double = 1),
// sum[e] = sum[e] + src[e].
constexpr int ACC_BATCH = 32;
struct AccumEntry {
    const void* src;
    double* sum;
    long long n;        // elements of the device buffer
    int pitch, nz;      // level pitch and real levels (1, 1 for a 2-D field)
    int src_double;
    int pad;
};
struct AccumBatch {
    AccumEntry e[ACC_BATCH];
    double w;
    int count;
};

}  // namespace trm
