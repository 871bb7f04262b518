// Launchers of score.hip (scoring a target panel with saved effects), called by
// the sgv_score_* entry points in capi.hip.
#pragma once
#include "common.h"

namespace sgv {

constexpr int SC_SLAB = 1024;   // markers per slab partial (by global marker index)
constexpr int SC_COLS = 16;     // columns per column group: the MFMA's N
// slab partials of one launch, in doubles (256 MB); a chunk with more slabs runs as
// several launches, which by the order contract changes no bit
constexpr int64_t SC_PART_MAX = (int64_t)32 * 1024 * 1024;

// tab[i][code] from the chunk's exact counts (cnt[i][4] as k_bed_stats fills them)
// and its {mean, sd}: mode 0 (x - mean) / sd, missing and markers without variance
// 0; mode 1 the A1 dosage 2 / 1 / 0, missing S1 / n_obs (0 if unobserved)
hipError_t launch_score_tab(int mode, const long long* d_cnt, const double* d_msd, int n,
                            double* d_tab, hipStream_t st);
// pk[i][c] = beta[(c0 + c) n + i] for c0 + c < ncol, else 0 (i < n, c < 16)
hipError_t launch_score_pack(const double* d_beta, int n, int ncol, int c0, double* d_pk,
                             hipStream_t st);
// part[s][smp][c] = sum over slab s's markers (i0 + 1024 s ..., at most nm in all) of
// tab_i[code_i,smp] pk[i][c], for nslab slabs; rows nsamp .. are not stored
hipError_t launch_score_mfma(const uint32_t* d_bits, int64_t stride_w, const double* d_tab,
                             const double* d_pk, int nm, int nslab, int nsamp, double* d_part,
                             hipStream_t st);
// S[smp][c] = (...((S + part[0]) + part[1]) ...) + part[nslab - 1]
hipError_t launch_score_sum(const double* d_part, int nslab, int nsamp, double* d_S,
                            hipStream_t st);

}  // namespace sgv
