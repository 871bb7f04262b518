// Multi-RHS symmetric LD pass on the f64 matrix cores.
//
// For 3..16 right-hand sides a VALU pass runs out of operands before HBM runs
// out of bytes: each stored R_ij feeds 2*NC FMAs whose P operands must sit in
// registers, so the VALU kernels (sym_pass.hip) re-read P or spill column
// partials through LDS at a multiple of the HBM traffic.  An MFMA takes ONE
// f64 of R and ONE f64 of P per lane and lets the matrix core do the register
// blocking.  Of the two f64 shapes, v_mfma_f64_4x4x4f64 (4 blocks of 4x4x4)
// costs 17 cycles for 256 MACs (~71 TF) and v_mfma_f64_16x16x4f64 140 cycles
// for 1024 (~47 TF) (tools/mfma_probe.hip; one accumulator chain: 44 / 184
// cycles per MFMA, 4 chains 18 / 144); the 4x4x4 form also needs only
// ceil(NC/4) column groups instead of padding to 16.  Per 16x32 sub-tile
// (4 KiB of R) the pass issues 16 * ceil(NC/4) of them (~270 cycles per group),
// under the ~1300-1500 cycles the same bytes take to arrive from HBM.
//
// 4x4x4 f64 lane maps (probed): block b = (l>>2)&3;
//   A_b[m][k] at lane 16k + 4b + m,  B_b[k][n] at lane 16k + 4b + n,
//   D_b[m][n] at lane 16m + 4b + n.
//
// Work items are strips (see k_sym_mfma): one 512-column chunk over several
// panels.  Row sums go to rowpart[item][256][NC] per (panel, chunk) item as in
// the VALU pass (class 1), column sums to colpart[strip][NC][512];
// k_sym_finalize_strip combines them.
//
// One workgroup per strip, NW waves; wave w owns chunk columns
// [w*512/NW, (w+1)*512/NW) and sweeps each panel's rows in 16-row groups.
// Each 16 x 32 sub-tile is loaded from HBM once, 16 B per lane:
//   col fragment  lane l: R[row 4a + (l>>4)][col pair (l&15), + e]   (a = 0..3)
//       A_b[m][k] = R[row k][pair 4b+m]: Dcol[pair][c] += R[j][i] P[j][c]
// and written to a per-wave LDS tile (16 x 32, XOR-swizzled 16-B pieces) from which
//   row fragment  lane l: R[row 4q + (l&3)][col pair (l>>4) + 4b, + e] (q = 0..3)
//       A_b[m][k] = R[row m][pair k+4b]: Drow[row][c] += R[j][i] P[i][c]
// is read back without bank conflicts.  Each 4x4x4 block contracts its own 4
// column pairs, so the 4 blocks' row partials are summed by two DPP row
// rotations per row group (fixed order), then over the waves through LDS (wave
// order).
// Dcol accumulates over all rows of the strip in registers; every order is fixed.
//
// The machinery of one wave -- operand and fragment loads, prefetch ring, tile,
// MFMA blocks, block reduction, partial stores -- is strip_wave.h's, one
// definition for the three 4x4x4 kernels here; a kernel's own text is how its
// waves divide a chunk and where their row sums meet.  k_sym_mfma16 keeps its
// own loads and ring (see there).
#include "strip_wave.h"

namespace sgv {

// Diagnostic build only (make EXTRA=-DSGV_MF_TRACE, tools/strip_trace.py): each
// workgroup (strip) of the last NC <= 8 MFMA pass records its start / end wall
// clock (100 MHz) and CU, to see how the launch fills the device.  Not in the
// product library.
#ifdef SGV_MF_TRACE
constexpr int MF_TRACE_MAX = 1 << 16;
__device__ unsigned long long g_mf_trace[3 * MF_TRACE_MAX];
#define MF_TRACE_BEGIN const unsigned long long tr_t0 = wall_clock64();
#define MF_TRACE_END                                                          \
  __syncthreads();                                                            \
  if (threadIdx.x == 0 && blockIdx.x < MF_TRACE_MAX) {                        \
    g_mf_trace[3 * blockIdx.x] = tr_t0;                                       \
    g_mf_trace[3 * blockIdx.x + 1] = wall_clock64();                          \
    g_mf_trace[3 * blockIdx.x + 2] = (unsigned long long)__smid();            \
  }
#else
#define MF_TRACE_BEGIN
#define MF_TRACE_END
#endif

constexpr int MF_CW = 512;   // chunk width (class 1 items)
constexpr int MF_LDP = 34;   // k_sym_mfma16's staging row pitch (doubles): conflict-free both ways

// Strips: a workgroup owns one 512-column chunk over up to S panels of one
// parity (g0, g0 + 2, ...: the panels whose items share that chunk's column
// alignment), so the column sums stay in registers across the panels and reach
// HBM once per strip instead of once per (panel, chunk) item.  The chunk's
// diagonal panel (r0 == c0) is the strip's last; its diagonal block (chunk
// columns 0..255, waves 0 and 1) must not feed the column sums, so those waves
// take zero B operands there (exact: R * 0 adds 0).  Row sums are still written
// per (panel, chunk) item.  Panel descriptors are wave-uniform (SGPRs).
// Each wave keeps its row sums of the whole panel in its own LDS rows
// (wrow[wave][row][4 NG]); the four waves' values are added, in wave order, once
// per panel when the item's row partials are written (one barrier pair per
// panel).
// DEF: the deferred row/column interleave (mfma_step_deferred); RAG, PP, T, LF
// and the row sets of NG = 2: StripWave.
template <int NG, int PD, bool RAG = false, bool DEF = false, bool PP = false, class T = double,
          int LF = 1>
__global__ __launch_bounds__(256, 2) void k_sym_mfma(const SymStrip* __restrict__ strips,
                                                     const SymItem* __restrict__ sitems,
                                                     const double* __restrict__ pk, int ncol,
                                                     double* __restrict__ rowpart,
                                                     double* __restrict__ colpart,
                                                     const int* __restrict__ run, int pks) {
  constexpr int NW = 4;            // waves 0 and 1 own the diagonal half of a chunk
  constexpr int WC = MF_CW / NW;   // columns per wave
  constexpr int NT = WC / 32;      // 32-column steps per wave
  typedef StripWave<NG, PP, T, LF, RAG> SW;
  constexpr int RW = SW::RW;
  __shared__ __attribute__((aligned(16))) double rowbuf[NW * SYM_H * RW];   // wrow
  __shared__ __attribute__((aligned(16))) double stg[NW][16 * 32];          // the waves' tiles
  const SymStrip sp = strips[blockIdx.x];
  if (run && !ldg(run)) return;   // no-op pass (pipelined CG past its stop test)
  MF_TRACE_BEGIN
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  SymItem cur = sitems[sp.it0];
  const int cw0 = wid * WC;
  const SW sw(lane, pk + (int64_t)cur.voff * pks, pks, cur.c0, sp.ncmax, cw0, cw0 < SYM_H);
  const int nta = min(NT, sw.steps_to(sw.ncc));
  double* sb = stg[wid];
  double brow[NT][2][NG];
  sw.load_brow(brow);
  double dcol[NT][2][NG];
  zero(dcol);

  uint64_t curb = SW::pbase(cur);
  FragRing<SW, PD, NT> ring;
  double bcn[SW::NB][NG];
  ring.prime(sw, curb, cur);
  sw.load_bcol(cur.r0, cur.H, sw.col_zero(cur.r0), 0, bcn);

#pragma unroll 1
  for (int s = 0; s < sp.npan; ++s) {                  // uniform over the workgroup
    const bool more = s + 1 < sp.npan;
    const SymItem nx = sitems[sp.it0 + (more ? s + 1 : s)];
    const uint64_t nxb = more ? SW::pbase(nx) : (uint64_t)sw.pkb;
    const int ng = (cur.H + 15) / 16;
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
      const NextGroup nxt = sw.next_group(g, ng, cur, curb, more, nx, nxb);
      double bcol[4][NG];
      sw.hand_bcol(bcn, bcol);
      double drow[4][NG];
      zero(drow);
      const bool colz = sw.col_zero(cur.r0);   // this panel's column B operands are 0
      // a band item narrower than its strip (its panel's last 256 columns): a
      // step wholly past its stored end adds only zeros -- skipped like the
      // steps past the chunk; per panel, so the deferred row MFMAs (DEF) know
      // the item's last active step
      const int ntp = RAG ? min(nta, sw.steps_to(cur.nc)) : nta;
      d2 rfb[DEF ? 2 : 1][4];                            // row fragments (DEF: this and the previous step)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        d2 cf[4];
        d2* rf = rfb[DEF ? (t & 1) : 0];
        ring.step(sw, t, g, curb, cur, nxt, bcn, cf);
        if (t >= ntp) continue;                        // wave-uniform: past the chunk / item
        if (RAG && cur.nc < sw.ncc) sw.band_zero(cur.nc, t, cf);   // uniform: a band item's stored end
        sw.tile_exchange(sb, cf, rf);
        // the MFMA burst at raised wave priority: the SIMD's other wave, whose
        // loads are in flight, takes the issue slots back when this one drains
        // (NC = 4/8 0.7-1.5 % faster per pass on two boxes; NC = 16 1 % slower,
        // not used there -- profiles/r02s10_prio_ab.txt)
        __builtin_amdgcn_s_setprio(1);
        if constexpr (DEF)
          mfma_step_deferred<NG, NT>(t, t == NT - 1 || t + 1 == ntp, colz, cf, rf,
                                     rfb[(t + 1) & 1], bcol, brow, dcol[t], drow);
        else
          mfma_step<NG>(colz, cf, rf, true, bcol, brow[t], dcol[t], drow);
        __builtin_amdgcn_s_setprio(0);
      }
      sw.reduce_blocks(drow, rowbuf + (wid * SYM_H + 16 * g) * RW);   // kept per wave for the panel
    }
    __syncthreads();
    panel_rows_out<NW, NW * 64, RW>(rowbuf, cur.H, ncol, rowpart + (int64_t)cur.item * SYM_H * ncol);
    __syncthreads();    // the waves' rows are read before the next panel writes them
    cur = nx;
    curb = nxb;
  }
  sw.template store_colpart<NT, MF_CW>(colpart + ((int64_t)sp.slot * ncol + sw.n4) * MF_CW + cw0,
                                       sw.pc, ncol, dcol);
  MF_TRACE_END
}

// Wave-pair form of k_sym_mfma (no band items): one 8-wave workgroup
// per strip, TWO waves per 128-column segment, each owning 64 columns (two
// 32-column steps).  Every sum is the 4-wave kernel's, bit for bit:
//  * a column's sum is one MFMA chain over the strip's rows in one wave, as
//    there (its wave only changed);
//  * a row's sum over a segment is the chain x0 y0 x1 y1 x2 y2 x3 y3 over the
//    segment's four steps: the first wave of the pair runs steps 0-1 from zero
//    and hands its accumulators (4 NG doubles per lane) through LDS to the
//    second, which continues with steps 2-3 -- the same MFMAs in the same order
//    -- then reduces the 4 blocks (DPP) and keeps the segment's panel row sums
//    (wrow), added over the 4 segments in order per panel as there.
// So a strip takes half the time on a workgroup holding a whole CU (8 waves, 1
// per CU: the same 2 waves per SIMD): a launch whose strips are few per slot
// (an 8-block share: ~2 strips of up to 8 panels per slot of the 4-wave form)
// drains with half the tail, with products identical to the 4-wave kernel's --
// the form can be chosen per partition.  One barrier per 16-row group: the
// hand-off (first wave: accumulators out before it; second wave: in after it,
// double-buffered by row-group parity).
// Waves s and s + 4 hold segment s (waves are dealt to SIMDs round-robin: the
// pair shares one SIMD, each SIMD runs one first and one second half); each
// pair syncs on its own LDS counters (the first wave up to HS - 1 row groups
// ahead, a ring of HS hand-off slots), barriers only at panel ends.  The other
// forms measured -- pair on two SIMDs, a barrier per row group -- were slower
// 
template <int NG, int PD, bool PP = false>
__global__ __launch_bounds__(512, 1) void k_sym_mfma_pair(const SymStrip* __restrict__ strips,
                                                          const SymItem* __restrict__ sitems,
                                                          const double* __restrict__ pk, int ncol,
                                                          double* __restrict__ rowpart,
                                                          double* __restrict__ colpart,
                                                          const int* __restrict__ run, int pks) {
  constexpr int NW = 8;
  constexpr int WC = 64;           // columns per wave
  constexpr int NT = WC / 32;      // 32-column steps per wave
  typedef StripWave<NG, PP> SW;
  constexpr int RW = SW::RW;
  __shared__ __attribute__((aligned(16))) double wrow[4 * SYM_H * RW];   // [segment][row][4 NG]
  constexpr int HS = 3;                                                    // hand-off slots
  __shared__ __attribute__((aligned(16))) double hand[HS][4][4 * NG][WAVE];   // [gg % HS][segment][r, q][lane]
  __shared__ int hready[4], hdone[4];   // row groups handed / taken per segment
  __shared__ __attribute__((aligned(16))) double stg[NW][16 * 32];
  const SymStrip sp = strips[blockIdx.x];
  if (run && !ldg(run)) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int seg = wid & 3;                               // 128-column segment
  const int h = wid >> 2;                                // half
  SymItem cur = sitems[sp.it0];
  const int cw0 = seg * 128 + h * WC;
  // dhalf: the 4-wave kernel's wave `seg`
  const SW sw(lane, pk + (int64_t)cur.voff * pks, pks, cur.c0, sp.ncmax, cw0, seg * 128 < SYM_H);
  // the segment's active 32-column steps (the 4-wave kernel's nta), this wave's share
  const int nta_seg = min(4, max(0, (sw.ncc - seg * 128 + 31) / 32));
  const int nta = min(NT, max(0, nta_seg - NT * h));
  double* sb = stg[wid];
  double brow[NT][2][NG];
  sw.load_brow(brow);
  double dcol[NT][2][NG];
  zero(dcol);

  uint64_t curb = SW::pbase(cur);
  FragRing<SW, PD, NT> ring;
  double bcn[SW::NB][NG];
  ring.prime(sw, curb, cur);
  sw.load_bcol(cur.r0, cur.H, sw.col_zero(cur.r0), 0, bcn);
  if (threadIdx.x < 4) hready[threadIdx.x] = hdone[threadIdx.x] = 0;
  __syncthreads();

  int gg = 0;
#pragma unroll 1
  for (int s = 0; s < sp.npan; ++s) {
    const bool more = s + 1 < sp.npan;
    const SymItem nx = sitems[sp.it0 + (more ? s + 1 : s)];
    const uint64_t nxb = more ? SW::pbase(nx) : (uint64_t)sw.pkb;
    const int ng = (cur.H + 15) / 16;
#pragma unroll 1
    for (int g = 0; g < ng; ++g, ++gg) {
      const NextGroup nxt = sw.next_group(g, ng, cur, curb, more, nx, nxb);
      double bcol[4][NG];
      sw.hand_bcol(bcn, bcol);
      double drow[4][NG];
      zero(drow);
      const bool colz = sw.col_zero(cur.r0);
      d2 rfs[NT][4];                                     // h = 1: row fragments, used after the hand-off
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        d2 cf[4];
        ring.step(sw, t, g, curb, cur, nxt, bcn, cf);
        if (t >= nta) continue;
        sw.tile_exchange(sb, cf, rfs[t]);
        __builtin_amdgcn_s_setprio(1);
        mfma_step<NG>(colz, cf, rfs[t], h == 0, bcol, brow[t], dcol[t], drow);   // h = 0: the chain's first half
        __builtin_amdgcn_s_setprio(0);
      }
      double* hs = &hand[gg % HS][seg][0][0];
      if (h == 0) {
        lds_wait_ge<__ATOMIC_ACQUIRE>(&hdone[seg], gg - HS + 1);   // slot gg % HS taken back
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NG; ++q) hs[(r * NG + q) * WAVE + lane] = drow[r][q];
        __hip_atomic_store(&hready[seg], gg + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if (h == 1) {
        lds_wait_ge<__ATOMIC_ACQUIRE>(&hready[seg], gg + 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < NG; ++q) drow[r][q] = hs[(r * NG + q) * WAVE + lane];
        __hip_atomic_store(&hdone[seg], gg + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (t < nta) row_mfma<NG>(rfs[t], brow[t], drow);   // the chain's second half
        __builtin_amdgcn_s_setprio(0);
        sw.reduce_blocks(drow, wrow + (seg * SYM_H + 16 * g) * RW);
      }
    }
    __syncthreads();   // the item's row sums: segments in order
    panel_rows_out<4, NW * 64, RW>(wrow, cur.H, ncol, rowpart + (int64_t)cur.item * SYM_H * ncol);
    __syncthreads();
    cur = nx;
    curb = nxb;
  }
  sw.template store_colpart<NT, MF_CW>(colpart + ((int64_t)sp.slot * ncol + sw.n4) * MF_CW + cw0,
                                       sw.pc, ncol, dcol);
}

// Wide strips (dense-triangle blocks, 3-8 columns): one 8-wave workgroup per
// strip of a 1,024-column chunk, one per CU; wave w owns chunk columns
// [128 w, 128 w + 128) and runs k_sym_mfma's DEF path on them (the same
// fragment loads, tile, operands, deferred row MFMAs and dummy loads).  An item
// is a (panel, 1,024-column chunk) pair, so a pass writes and reads back half
// the row partials of the 512-column forms.
// Row sums: per 16-row group each wave reduces its 4 blocks (DPP), writes its
// 16 x 4 NG sums into hand-off buffer gg mod MFW_RD and bumps the buffer's
// arrival counter; wave gg mod nact adds the segments in wave order and writes
// the group's 16 x ncol sums straight to rowpart (band_walk.hip's pattern:
// wavefront-scope fences, workgroup-scope relaxed counters; a wave runs up to
// MFW_RD - 1 row groups ahead of the slowest).  No barrier after the start.
// idle: a wave whose whole segment lies past the strip's last column (the
// ragged last chunk of a column class) would add exact zeros; it leaves at the
// start and the combine counts the nact waves left.
// Column sums: one chain per column over the strip's rows, as k_sym_mfma.
// The summation order differs from the 512-column forms' (a row's item sums
// are eight 128-column segments over 1,024 columns), so the bits do: which
// form a block takes is a function of the block alone (ldplan.hip).
constexpr int MFW_RD = 4;   // hand-off buffers (32 KiB at NG = 2, beside 32 KiB of tiles)
template <int NG, int PD, bool PP = false>
__global__ __launch_bounds__(512, 1) void k_sym_mfma_wide(const SymStrip* __restrict__ strips,
                                                          const SymItem* __restrict__ sitems,
                                                          const double* __restrict__ pk, int ncol,
                                                          double* __restrict__ rowpart,
                                                          double* __restrict__ colpart,
                                                          const int* __restrict__ run, int idle) {
  constexpr int NW = 8;
  constexpr int WC = MFW_CW / NW;  // columns per wave
  constexpr int NT = WC / 32;      // 32-column steps per wave
  typedef StripWave<NG, PP> SW;
  constexpr int RW = SW::RW;
  __shared__ __attribute__((aligned(16))) double hand[MFW_RD][NW][16 * RW];
  __shared__ int hready[MFW_RD], hdone[MFW_RD];   // writes into / combines of each buffer
  __shared__ __attribute__((aligned(16))) double stg[NW][16 * 32];
  const SymStrip sp = strips[blockIdx.x];
  if (run && !ldg(run)) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  SymItem cur = sitems[sp.it0];
  constexpr int PKS = 4 * NG;      // Pk row stride (k_pack)
  const int cw0 = wid * WC;
  // dhalf: waves 0 and 1, the diagonal block
  const SW sw(lane, pk + (int64_t)cur.voff * PKS, PKS, cur.c0, sp.ncmax, cw0, cw0 < SYM_H);
  const int nta = min(NT, sw.steps_to(sw.ncc));
  // waves with columns inside the strip
  const int nact = idle ? min(NW, (sw.ncc + WC - 1) / WC) : NW;
  if (threadIdx.x < MFW_RD) hready[threadIdx.x] = hdone[threadIdx.x] = 0;
  __syncthreads();
  if (wid >= nact) return;
  double* sb = stg[wid];
  double brow[NT][2][NG];
  sw.load_brow(brow);
  double dcol[NT][2][NG];
  zero(dcol);

  uint64_t curb = SW::pbase(cur);
  FragRing<SW, PD, NT> ring;
  double bcn[SW::NB][NG];
  ring.prime(sw, curb, cur);
  sw.load_bcol(cur.r0, cur.H, sw.col_zero(cur.r0), 0, bcn);

  // this lane's place in the strip's colpart slot, kept in vector registers
  // over the loops (the scalar file is full: no spills)
  double* outp = colpart + ((int64_t)sp.slot * ncol + sw.n4) * MFW_CW + cw0 + 2 * sw.pc;
  asm volatile("" : "+v"(outp));
  int gg = 0;   // row groups done: buffer gg % MFW_RD, round gg / MFW_RD
#pragma unroll 1
  for (int s = 0; s < sp.npan; ++s) {                  // uniform over the workgroup
    const bool more = s + 1 < sp.npan;
    const SymItem nx = sitems[sp.it0 + (more ? s + 1 : s)];
    const uint64_t nxb = more ? SW::pbase(nx) : (uint64_t)sw.pkb;
    const int ng = (cur.H + 15) / 16;
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
      const NextGroup nxt = sw.next_group(g, ng, cur, curb, more, nx, nxb);
      double bcol[4][NG];
      sw.hand_bcol(bcn, bcol);
      double drow[4][NG];
      zero(drow);
      const bool colz = sw.col_zero(cur.r0);   // this panel's column B operands are 0
      d2 rfb[2][4];                               // row fragments: this and the previous step
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        d2 cf[4];
        ring.step(sw, t, g, curb, cur, nxt, bcn, cf);
        if (t >= nta) continue;                        // wave-uniform: past the chunk
        sw.tile_exchange(sb, cf, rfb[t & 1]);
        __builtin_amdgcn_s_setprio(1);
        mfma_step_deferred<NG, NT>(t, t == NT - 1 || t + 1 == nta, colz, cf, rfb[t & 1],
                                   rfb[(t + 1) & 1], bcol, brow, dcol[t], drow);
        __builtin_amdgcn_s_setprio(0);
      }
      // the row group's row sums: 4 blocks (DPP), handed to the combining wave
      const int hs = gg % MFW_RD, gen = gg / MFW_RD;
      lds_wait_ge<__ATOMIC_RELAXED>(&hdone[hs], gen);   // buffer hs free (its last round combined)
      sw.reduce_blocks(drow, hand[hs][wid]);
      // a wave's DS operations execute in order, so the counter's add lands
      // after the row sums; the fences keep the compiler's order and wait for
      // nothing (the fragments stay in flight)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      if (lane == 0)
        __hip_atomic_fetch_add(&hready[hs], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      // the panel's row group g is combined by wave g mod 8 (wave 0 for an idle one)
      if (wid == ((g & (NW - 1)) < nact ? (g & (NW - 1)) : 0)) {   // the waves in order
        lds_wait_ge<__ATOMIC_RELAXED>(&hready[hs], nact * (gen + 1));
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double* dst = rowpart + ((int64_t)cur.item * SYM_H + 16 * g) * ncol;
#pragma unroll
        for (int k = 0; k < (16 * RW + WAVE - 1) / WAVE; ++k) {
          const int e = lane + WAVE * k;
          if (e < 16 * RW) {
            const int row = e / RW, cc = e - row * RW;
            const double* rr = &hand[hs][0][0] + e;
            double v = rr[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) {   // branch-free: a wave that left adds 0
              const double x = rr[w * 16 * RW];
              v += w < nact ? x : 0.0;
            }
            if (16 * g + row < cur.H && cc < ncol) dst[row * ncol + cc] = v;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (lane == 0)
          __hip_atomic_store(&hdone[hs], gen + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      ++gg;
    }
    cur = nx;
    curb = nxb;
  }
  // outp already holds the lane's pair: p = 0
  sw.template store_colpart<NT, MFW_CW>(outp, 0, ncol, dcol);
}

// 13..16 right-hand sides: v_mfma_f64_16x16x4f64 (one 16-column group, 140
// cycles per 16x16x4) keeps fewer accumulators and B operands in registers
// than four 4x4x4 groups, which spill at 4 waves.  Same strips as above:
//   col fragment -> A (m = column, k = row); LDS tile -> row fragment
//   lane l: R[row (l&15)][col 8s + 2(l>>4) + e] -> A (m = row, k = column);
//   16x16x4 f64 C/D layout (cdna_hip_programming.md): D[(l>>4) + 4r][l & 15].
typedef double d4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
// This kernel keeps its own text of the loads, the ring and the next-group
// selects (StripWave::load_cf / load_bcol / band_zero, FragRing, next_group in
// strip_wave.h, with one column group across 16 lanes and no row sets): at
// 252-255 VGPRs its schedule turns on the order of its statements.  On the
// shared forms the f32 16-B ragged instance went from 255 to 256 VGPRs and the
// 16-column f32 band pass (M = 1e6, bw = 1,000) from 2.2525 to 2.2874 ms
// (medians of 5, builds alternating; the parent's spread 0.0133:
// profiles/strip_refactor/speed_band_f32_rerun5.jsonl); with this text every
// instance compiles to the instruction stream it had.
// TB: the row-part B operands of the last TB steps kept in LDS (8 TB doubles per
// lane, 4 TB KiB per wave, read back per step as 4 x 16 B) instead of registers
template <int PD, bool RAG = false, int TB = 0, class T = double, int LF = 1>
__global__ __launch_bounds__(256, 2) void k_sym_mfma16(const SymStrip* __restrict__ strips,
                                                     const SymItem* __restrict__ sitems,
                                                     const double* __restrict__ pk, int ncol,
                                                     double* __restrict__ rowpart,
                                                     double* __restrict__ colpart,
                                                     const int* __restrict__ run) {
  constexpr int LDP = MF_LDP;
  constexpr int MF_WC = MF_CW / 4; // columns per wave
  constexpr int MF_NT = MF_WC / 32;
  constexpr bool W4 = LF == 2;        // 16-B loads of float panels (frag_col)
  static_assert(!W4 || (sizeof(T) == 4 && PD == 2 && MF_NT % 2 == 0), "LF = 2: float, two super-steps");
  typedef typename std::conditional<W4, f4, typename Frag<T>::raw>::type RV;   // a fragment as loaded
  constexpr int RD = W4 ? MF_NT / 2 : PD;
  __shared__ double red[2][4][256];
  __shared__ __attribute__((aligned(16))) double stg[4][16 * LDP];
  constexpr bool BL = TB > 0;
  __shared__ __attribute__((aligned(16))) double bls[BL ? 4 : 1][BL ? TB * 4 : 1][WAVE][2];
  const SymStrip sp = strips[blockIdx.x];
  if (run && !ldg(run)) return;   // no-op pass (pipelined CG past its stop test)
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lo = lane & 15, hi = lane >> 4;
  SymItem cur = sitems[sp.it0];
  const int c0 = cur.c0, ncc = sp.ncmax;
  const double* pkb = pk + (int64_t)cur.voff * 16;    // Pk of this block (block-relative index)
  const int cw0 = wid * MF_WC;                         // first chunk column of this wave
  const bool dhalf = cw0 < SYM_H;
  const int nta = W4 ? min(MF_NT, max(0, steps_upto<LF>(ncc - cw0)))
                     : min(MF_NT, max(0, (ncc - cw0 + 31) / 32));   // StripWave::steps_to

  double* sb = stg[wid];
  // row-part B operands (P at this wave's columns), reused by every row group
  double brow[MF_NT - TB][4][2];
#pragma unroll
  for (int t = 0; t < MF_NT; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int col = W4 ? cw0 + frag_col<LF>(t, 4 * s + hi) + e   // pair 4 s + hi
                           : cw0 + 32 * t + 8 * s + 2 * hi + e;
        const double v = ldg(pkb + (int64_t)(c0 + (col < ncc ? col : 0)) * 16 + lo);
        if (t < MF_NT - TB) brow[t < MF_NT - TB ? t : 0][s][e] = col < ncc ? v : 0.0;
        else if constexpr (BL) bls[wid][(t - (MF_NT - TB)) * 4 + s][lane][e] = col < ncc ? v : 0.0;
      }
  d4 dcol[MF_NT][2];
#pragma unroll
  for (int t = 0; t < MF_NT; ++t) dcol[t][0] = dcol[t][1] = d4{0.0, 0.0, 0.0, 0.0};

  auto load_cf = [&](uint64_t b0, int64_t ws, int H, int nci, int g, int t, RV* cf) {
    asm volatile("" : "+s"(b0));
    const int xc = W4 ? cw0 + 64 * t + 4 * lo : cw0 + 32 * t + 2 * lo;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int rB = 16 * g + 4 * a + hi;
      const T* row = (const T*)b0 + (int64_t)(rB < H ? rB : H - 1) * ws;
      cf[a] = ldg_nt((const RV*)(row + (xc < (RAG ? nci : ncc) ? xc : 0)));
    }
  };
  auto band_zero = [&](int nci, int t, d2* cf) {
    const int xc = W4 ? cw0 + frag_col<LF>(t, lo) : cw0 + 32 * t + 2 * lo;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      cf[a].x = xc < nci ? cf[a].x : 0.0;
      cf[a].y = xc + 1 < nci ? cf[a].y : 0.0;
    }
  };
  auto load_bcol = [&](int r0, int H, bool zero, int g, double* bc) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int rB = 16 * g + 4 * a + hi;
      const double v = ldg(pkb + (int64_t)(r0 + (rB < H ? rB : 0)) * 16 + lo);
      bc[a] = (rB < H && !zero) ? v : 0.0;
    }
  };
  auto pbase = [&](const SymItem& x) { return (uint64_t)((const T*)x.P + (x.c0 - x.r0)); };

  static_assert(PD >= 1 && PD <= MF_NT && MF_NT % PD == 0, "prefetch depth divides the steps");
  uint64_t curb = pbase(cur);
  RV cfq[RD][4];                                       // ring of PD steps in flight per wave
  double bcn[4];
#pragma unroll
  for (int p = 0; p < RD; ++p) load_cf(curb, cur.w, cur.H, cur.nc, 0, p, cfq[p]);
  load_bcol(cur.r0, cur.H, dhalf && cur.r0 == c0, 0, bcn);

  int gg = 0;
#pragma unroll 1
  for (int s = 0; s < sp.npan; ++s) {
    const bool more = s + 1 < sp.npan;
    const SymItem nx = sitems[sp.it0 + (more ? s + 1 : s)];
    const uint64_t nxb = more ? pbase(nx) : (uint64_t)pkb;
    const int ng = (cur.H + 15) / 16;
#pragma unroll 1
    for (int g = 0; g < ng; ++g, ++gg) {
      const bool same = g + 1 < ng;
      const uint64_t gb = same ? curb : nxb;
      const int64_t gw = same ? cur.w : (more ? nx.w : 0);
      const int gH = same ? cur.H : (more ? nx.H : 1);
      const int gn = same ? g + 1 : 0;
      const int gnc = same ? cur.nc : nx.nc;
      const int gr0 = same ? cur.r0 : nx.r0;
      const bool gz = dhalf && gr0 == c0;
      double bcol[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) bcol[a] = bcn[a];
      d4 drow0 = d4{0.0, 0.0, 0.0, 0.0}, drow1 = drow0;
      const bool colz = dhalf && cur.r0 == c0;
      d2 cfw[W4 ? 2 : 1][4];                           // LF = 2: a super-step's two steps, widened
#pragma unroll
      for (int t = 0; t < MF_NT; ++t) {
        d2 cf[4], rf[4];
        const int slot = t % PD;                       // compile-time after unrolling
        if constexpr (W4) {
          if ((t & 1) == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const f4 v = cfq[t >> 1][a];
              cfw[0][a] = d2{(double)v.x, (double)v.y};
              cfw[1][a] = d2{(double)v.z, (double)v.w};
            }
            load_cf(gb, gw, gH, gnc, gn, t >> 1, cfq[t >> 1]);
            if (t + PD == MF_NT) load_bcol(gr0, gH, gz, gn, bcn);
          }
#pragma unroll
          for (int a = 0; a < 4; ++a) cf[a] = cfw[t & 1][a];
        } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) cf[a] = Frag<T>::widen(cfq[slot][a]);
        // step + PD goes out here, ahead of this step's LDS and MFMA work
        if (t + PD < MF_NT) {
          load_cf(curb, cur.w, cur.H, cur.nc, g, t + PD, cfq[slot]);
        } else {
          load_cf(gb, gw, gH, gnc, gn, t + PD - MF_NT, cfq[slot]);
          if (t + PD == MF_NT) load_bcol(gr0, gH, gz, gn, bcn);
        }
        }
        if (t >= nta) continue;
        if (RAG && cw0 + (W4 ? 64 * (t >> 1) : 32 * t) >= cur.nc) continue;   // wholly past the item
        if (RAG && cur.nc < ncc) band_zero(cur.nc, t, cf);
        lds_order();                                   // previous step's tile reads done
#pragma unroll
        for (int a = 0; a < 4; ++a) *(d2*)(sb + (4 * a + hi) * LDP + 2 * lo) = cf[a];
        lds_order();                                   // tile written
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) rf[s2] = *(const d2*)(sb + lo * LDP + 8 * s2 + 2 * hi);
        d2 bt[4];   // this step's row-part B operands
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
          if (t < MF_NT - TB) bt[s2] = d2{brow[t < MF_NT - TB ? t : 0][s2][0], brow[t < MF_NT - TB ? t : 0][s2][1]};
          else if constexpr (BL) bt[s2] = *(const d2*)&bls[wid][(t - (MF_NT - TB)) * 4 + s2][lane][0];
        }
        if (!colz) {
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            dcol[t][0] = MFMA16(cf[a].x, bcol[a], dcol[t][0]);
            dcol[t][1] = MFMA16(cf[a].y, bcol[a], dcol[t][1]);
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
          drow0 = MFMA16(rf[s2].x, bt[s2].x, drow0);
          drow1 = MFMA16(rf[s2].y, bt[s2].y, drow1);
        }
      }
      // row sums of this 16-row group: waves 0..3 in order
      double* rb = red[gg & 1][wid];
#pragma unroll
      for (int r = 0; r < 4; ++r) rb[((hi + 4 * r) << 4) + lo] = drow0[r] + drow1[r];
      __syncthreads();
      {
        const int t = threadIdx.x, row = t >> 4, cc = t & 15;
        const double v = ((red[gg & 1][0][t] + red[gg & 1][1][t]) + red[gg & 1][2][t]) +
                         red[gg & 1][3][t];
        if (16 * g + row < cur.H && cc < ncol)
          rowpart[((int64_t)cur.item * SYM_H + 16 * g + row) * ncol + cc] = v;
      }
    }
    cur = nx;
    curb = nxb;
  }

  // column sums over the strip's panels (whole slot, 16-B stores)
  if (lo < ncol) {
    double* out = colpart + ((int64_t)sp.slot * ncol + lo) * MF_CW;
#pragma unroll
    for (int t = 0; t < MF_NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if constexpr (W4)
          *(d2*)(out + cw0 + frag_col<LF>(t, hi + 4 * r)) = d2{dcol[t][0][r], dcol[t][1][r]};
        else
          *(d2*)(out + cw0 + 32 * t + 2 * (hi + 4 * r)) = d2{dcol[t][0][r], dcol[t][1][r]};
  }
}

// one workgroup per panel, FIN_Q threads per row (row t = r0 + (thread & 255),
// part q = thread >> 8): part q sums the panel's row parts item_begin + q, + 2q,
// ..., then the strips own_sb + q, ... of the own-parity chunk (column offset
// t) and oth_sb + q, ... of the other-parity chunk (offset 256 + t); parts are
// added in order (fin_epilogue) -- fixed order throughout
template <int NC>
__global__ __launch_bounds__(256 * FIN_Q) void k_sym_finalize_strip(
    const SymPanel* __restrict__ panels, PassArgs pa, const double* __restrict__ rowpart,
    const double* __restrict__ colpart, double* __restrict__ partials) {
  const SymPanel pn = panels[blockIdx.x];
  if (pa.run && !ldg(pa.run)) return;
  FinPre<NC> pre;
  fin_prefetch<NC>(pn, pa, pre);
  const int t = threadIdx.x & 255, q = threadIdx.x >> 8;
  const int tr = t < pn.H ? t : 0;
  double y[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) y[c] = 0.0;
#pragma unroll 4
  for (int itm = pn.item_begin + q; itm < pn.item_end; itm += FIN_Q) {
    const double* rp = rowpart + ((int64_t)itm * SYM_H + t) * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] += ldg(rp + c);
  }
#pragma unroll 4
  for (int sl = pn.own_sb + q; sl < pn.own_se; sl += FIN_Q) {
    const double* cp = colpart + (int64_t)sl * NC * MF_CW + tr;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] += ldg(cp + c * MF_CW);
  }
#pragma unroll 4
  for (int sl = pn.oth_sb + q; sl < pn.oth_se; sl += FIN_Q) {
    const double* cp = colpart + (int64_t)sl * NC * MF_CW + SYM_H + tr;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] += ldg(cp + c * MF_CW);
  }
  fin_epilogue<NC>(pn, pa, y, partials, pre);
}

// The same sums with one thread per panel row holding all FIN_Q parts in
// registers (part q: items item_begin + q, + FIN_Q, ..., then the own and other
// strips q, q + FIN_Q, ...; parts added in order 0..3, then the coupling sum,
// the epilogue and the panel's partial dots: wave butterfly over the same 64
// rows, waves in order) -- every addition of k_sym_finalize_strip in the same
// order, so bitwise the same outputs, in a 256-thread workgroup without the
// cross-part LDS exchange (a band panel has ~3 items and 2 strips: the
// 1024-thread form spends its time starting waves)
template <int NC>
__global__ __launch_bounds__(256) void k_sym_finalize_strip1(
    const SymPanel* __restrict__ panels, PassArgs pa, const double* __restrict__ rowpart,
    const double* __restrict__ colpart, double* __restrict__ partials) {
  const SymPanel pn = panels[blockIdx.x];
  if (pa.run && !ldg(pa.run)) return;
  const int t = threadIdx.x;
  const bool row = t < pn.H;
  const int tr = row ? t : 0;
  const int64_t idx = pn.voff + pn.r0 + tr;
  double in[NC], dt[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    in[c] = pa.in[c][idx];
    dt[c] = pa.dot[c] ? pa.dot[c][idx] : 0.0;
  }
  double y[FIN_Q][NC];
#pragma unroll
  for (int q = 0; q < FIN_Q; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) y[q][c] = 0.0;
#pragma unroll
  for (int q = 0; q < FIN_Q; ++q) {
#pragma unroll 2
    for (int itm = pn.item_begin + q; itm < pn.item_end; itm += FIN_Q) {
      const double* rp = rowpart + ((int64_t)itm * SYM_H + t) * NC;
#pragma unroll
      for (int c = 0; c < NC; ++c) y[q][c] += ldg(rp + c);
    }
#pragma unroll 2
    for (int sl = pn.own_sb + q; sl < pn.own_se; sl += FIN_Q) {
      const double* cp = colpart + (int64_t)sl * NC * MF_CW + tr;
#pragma unroll
      for (int c = 0; c < NC; ++c) y[q][c] += ldg(cp + c * MF_CW);
    }
#pragma unroll 2
    for (int sl = pn.oth_sb + q; sl < pn.oth_se; sl += FIN_Q) {
      const double* cp = colpart + (int64_t)sl * NC * MF_CW + SYM_H + tr;
#pragma unroll
      for (int c = 0; c < NC; ++c) y[q][c] += ldg(cp + c * MF_CW);
    }
  }
  __shared__ double s_w[4][NC];
  const int lane = t & (WAVE - 1), wid = t / WAVE;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double v = y[0][c];
#pragma unroll
    for (int p = 1; p < FIN_Q; ++p) v += y[p][c];
    if (pn.cp >= 0) v += pa.cpbuf[((int64_t)pn.cp * 256 + t) * NC + c];   // coupled pieces
    double acc = 0.0;
    if (row) {
      const double o = pa.c1[c] * v + pa.c2[c] * in[c];
      pa.out[c][idx] = o;
      if (pa.yout[c]) pa.yout[c][idx] = pa.ys1 * v + pa.ys0 * in[c];
      if (pa.dot[c]) acc = dt[c] * o;
    }
    const double sm = wave_sum(acc);
    if (lane == 0) s_w[wid][c] = sm;
  }
  __syncthreads();
  if (t < NC) partials[(int64_t)pn.part * NC + t] = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
}

// k_sym_finalize_strip over the wide tables: part q sums the panel's
// 1,024-column items item_begin + q, + FIN_Q, ..., then for k = 0..3 the strips
// sb[k] + q, + FIN_Q, ... of the chunk starting k panels before this one (row
// offset 256 k); parts added in order (fin_epilogue) -- fixed order throughout
template <int NC>
__global__ __launch_bounds__(256 * FIN_Q) void k_sym_finalize_wide(
    const SymPanelW* __restrict__ panels, PassArgs pa, const double* __restrict__ rowpart,
    const double* __restrict__ colpart, double* __restrict__ partials) {
  const SymPanelW pw = panels[blockIdx.x];
  const SymPanel& pn = pw.p;
  if (pa.run && !ldg(pa.run)) return;
  FinPre<NC> pre;
  fin_prefetch<NC>(pn, pa, pre);
  const int t = threadIdx.x & 255, q = threadIdx.x >> 8;
  const int tr = t < pn.H ? t : 0;
  double y[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) y[c] = 0.0;
#pragma unroll 4
  for (int itm = pn.item_begin + q; itm < pn.item_end; itm += FIN_Q) {
    const double* rp = rowpart + ((int64_t)itm * SYM_H + t) * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] += ldg(rp + c);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll 4
    for (int sl = pw.sb[k] + q; sl < pw.se[k]; sl += FIN_Q) {
      const double* cp = colpart + (int64_t)sl * NC * MFW_CW + SYM_H * k + tr;
#pragma unroll
      for (int c = 0; c < NC; ++c) y[c] += ldg(cp + c * MFW_CW);
    }
  }
  fin_epilogue<NC>(pn, pa, y, partials, pre);
}

// Pk[i][c] = in[c][i] for c < ncol, 0 for ncol <= c < PKS (i over the padded
// vector).  PKS = the columns the pass kernel's groups read: 4 (NC <= 4), 8
// (NC <= 8), 16 -- a row is one cache line's worth of what is read, so the
// pass's Pk reads (L2 misses on M = 1e6) carry no unused columns
// PAIRED (PKS = 8, the 5-8-column band walks): slot p holds column
// 4 (p & 1) + (p >> 1), so the walk's lane n4 reads its columns n4 and 4 + n4
// as one 16-B load
// One thread per row: the column reads are coalesced over the threads, the
// row is written as 16-B stores.
template <int PKS, bool PAIRED = false>
__global__ __launch_bounds__(256) void k_pack(PassArgs pa, int ncol, int64_t mpad,
                                              double* __restrict__ pk) {
  if (pa.run && !ldg(pa.run)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mpad) return;
  double v[PKS];
#pragma unroll
  for (int p = 0; p < PKS; ++p) {
    const int c = PAIRED ? 4 * (p & 1) + (p >> 1) : p;
    v[p] = c < ncol ? pa.in[c][i] : 0.0;
  }
  d2* row = (d2*)(pk + i * PKS);
#pragma unroll
  for (int p = 0; p < PKS; p += 2) row[p / 2] = d2{v[p], v[p + 1]};
}

// ragged: some strip item stops short of its strip's widest (band blocks):
// the RAG kernels, without the deferred row MFMAs (even there,
// profiles/r04/band2_ab.jsonl).  pair: the wave-pair kernel.
// f32 (the tables' panels hold floats): the float instances of the same two
// 4-wave kernels -- RAG for band plans, DEF otherwise; there is no float pair form.
// form: the float kernels' load form.  pair, form, pks and the finalize's form
// are pass_form's (pass_form.cpp, with what was measured).

// The (stored type, load form, ragged) instance of a 4-wave strip kernel a
// launch takes, chosen once: f(StripInst<T, LF, RAG>{}) launches it.
template <class T, int LF, bool RAG>
struct StripInst {
  typedef T elem;
  static constexpr int lf = LF;
  static constexpr bool rag = RAG;
};
template <class F>
static void with_strip_inst(bool f32, bool ragged, int form, F f) {
  if (f32 && form == 2)
    ragged ? f(StripInst<float, 2, true>{}) : f(StripInst<float, 2, false>{});
  else if (f32)
    ragged ? f(StripInst<float, 1, true>{}) : f(StripInst<float, 1, false>{});
  else
    ragged ? f(StripInst<double, 1, true>{}) : f(StripInst<double, 1, false>{});
}

template <int NG, bool PP = false>
static void launch_mf(const SymStrip* d_strips, int nstrips, const SymItem* d_sitems,
                      const double* d_pk, int nc, double* rowpart, double* colpart,
                      const int* run, int pks, bool ragged, bool pair, bool f32, int form,
                      hipStream_t st) {
  // prefetch depth 2 measured best (PD 1/2/4: 11.64/11.16/12.27 ms at NC=4, M=1e6)
  if (pair)
    hipLaunchKernelGGL((k_sym_mfma_pair<NG, 2, PP>), dim3(nstrips), dim3(512), 0, st, d_strips,
                       d_sitems, d_pk, nc, rowpart, colpart, run, pks);
  else
    with_strip_inst(f32, ragged, form, [&](auto i) {
      typedef decltype(i) I;   // RAG for band plans, DEF otherwise
      hipLaunchKernelGGL((k_sym_mfma<NG, 2, I::rag, !I::rag, PP, typename I::elem, I::lf>),
                         dim3(nstrips), dim3(256), 0, st, d_strips, d_sitems, d_pk, nc, rowpart,
                         colpart, run, pks);
    });
}

hipError_t launch_pk(const PassArgs& pa, int nc, int64_t mpad, double* d_pk, int pks, bool paired,
                     hipStream_t st) {
  if (nc < 1 || nc > 16) return hipErrorInvalidValue;
  if ((pks != 4 && pks != 8 && pks != 16) || nc > pks) return hipErrorInvalidValue;
  const dim3 pg((unsigned)((mpad + 255) / 256));
  if (pks == 4)
    hipLaunchKernelGGL(k_pack<4>, pg, dim3(256), 0, st, pa, nc, mpad, d_pk);
  else if (pks == 8 && paired)
    hipLaunchKernelGGL((k_pack<8, true>), pg, dim3(256), 0, st, pa, nc, mpad, d_pk);
  else if (pks == 8)
    hipLaunchKernelGGL(k_pack<8>, pg, dim3(256), 0, st, pa, nc, mpad, d_pk);
  else
    hipLaunchKernelGGL(k_pack<16>, pg, dim3(256), 0, st, pa, nc, mpad, d_pk);
  return hipGetLastError();
}

hipError_t launch_sym_mfma(int nc, const SymStrip* d_strips, int nstrips, const SymItem* d_sitems,
                           const PassArgs& pa, const double* d_pk, int pks, double* rowpart,
                           double* colpart, bool ragged, bool pair, int bits, int form,
                           hipStream_t st) {
  if (nc < 1 || nc > 16) return hipErrorInvalidValue;
  if (bits != 64 && bits != 32) return hipErrorInvalidValue;
  const bool f32 = bits == 32;
  if (f32 && pair) return hipErrorInvalidValue;   // no float instance of the pair form
  if (pair && (ragged || nc > 8)) return hipErrorInvalidValue;   // nor a ragged or 16-column one
  if (nstrips <= 0) return hipSuccess;
  // 9..16 columns: one 16x16x4 group beats three/four 4x4x4 groups (register
  // pressure) and two 8-column wave sets of the 4x4x4 kernel in one 8-wave
  // workgroup re-reading the same R with the default cache policy (+33 %,
  // profiles/r03/s4/mf_sets_ab.jsonl) and three / four 4x4x4 groups at one wave
  // per SIMD with the deferred row MFMAs (+13 % / +28 %, ng4_ab.jsonl):
  // measured in DESIGN.md.  Prefetch depth 2 (with every row operand in
  // registers it spilled 3 / 7 VGPRs on dense / band plans and was still faster
  // than depth 1: profiles/r03/s4/mf16_pd_ab.jsonl, profiles/r04/band2_ab.jsonl).
  // Round 6 measured the spill-free forms on one
  // box (profiles/r06/mf16_forms_ab.jsonl, _bench_c5conv.jsonl): depth 1 (236
  // VGPRs) +1.5-2 % per pass, 8 waves of 64 columns per workgroup (188 VGPRs)
  // +8 %, and the row part on 4x4x4 MFMA in that form (210 VGPRs) +18 % -- the
  // 8-wave row-sum combine and the 4x4x4 form's DPP reductions and 4x the MFMA
  // issues cost more than they save; the spill-free form kept is the row
  // operands of the last step(s) in LDS (below).
  switch ((nc + 3) / 4) {
    case 1:
      launch_mf<1>(d_strips, nstrips, d_sitems, d_pk, nc, rowpart, colpart, pa.run, pks, ragged,
                   pair, f32, form, st);
      break;
    case 2:   // Pk paired
      launch_mf<2, true>(d_strips, nstrips, d_sitems, d_pk, nc, rowpart, colpart, pa.run, pks,
                         ragged, pair, f32, form, st);
      break;
    default:
      // the row operands of the last steps in LDS, so nothing spills (256 VGPRs
      // with 3 / 7 spilled before): band plans the last 2 steps (-0.6 % per
      // 16-column band pass), dense plans the last one (even; 2 steps there +2 %)
      // -- profiles/r06/mf16_bl_*.jsonl, mf16_tb_*.jsonl; products bitwise equal
      with_strip_inst(f32, ragged, form, [&](auto i) {
        typedef decltype(i) I;
        hipLaunchKernelGGL((k_sym_mfma16<2, I::rag, I::rag ? 2 : 1, typename I::elem, I::lf>),
                           dim3(nstrips), dim3(256), 0, st, d_strips, d_sitems, d_pk, nc, rowpart,
                           colpart, pa.run);
      });
      break;
  }
  return hipGetLastError();
}

hipError_t launch_sym_mfma_wide(int nc, const SymStrip* d_strips, int nstrips,
                                const SymItem* d_sitems, const PassArgs& pa, const double* d_pk,
                                double* rowpart, double* colpart, bool idle_exit, hipStream_t st) {
  if (nc < 3 || nc > 8) return hipErrorInvalidValue;
  if (nstrips <= 0) return hipSuccess;
  if (nc <= 4)
    hipLaunchKernelGGL((k_sym_mfma_wide<1, 2>), dim3(nstrips), dim3(512), 0, st, d_strips,
                       d_sitems, d_pk, nc, rowpart, colpart, pa.run, idle_exit ? 1 : 0);
  else   // Pk paired
    hipLaunchKernelGGL((k_sym_mfma_wide<2, 2, true>), dim3(nstrips), dim3(512), 0, st, d_strips,
                       d_sitems, d_pk, nc, rowpart, colpart, pa.run, idle_exit ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_sym_finalize_wide(int nc, const SymPanelW* d_panels, int npanels,
                                    const PassArgs& pa, const double* rowpart,
                                    const double* colpart, double* partials, hipStream_t st) {
  if (npanels <= 0) return hipSuccess;
#define FINW_CASE(N)                                                                         \
  case N:                                                                                    \
    hipLaunchKernelGGL(k_sym_finalize_wide<N>, dim3(npanels), dim3(256 * FIN_Q), 0, st,      \
                       d_panels, pa, rowpart, colpart, partials);                            \
    break;
  switch (nc) {
    FINW_CASE(3) FINW_CASE(4) FINW_CASE(5) FINW_CASE(6) FINW_CASE(7) FINW_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef FINW_CASE
  return hipGetLastError();
}

#ifdef SGV_MF_TRACE
extern "C" int sgv_diag_mf_trace(unsigned long long* out, int n) {
  if (n > MF_TRACE_MAX) n = MF_TRACE_MAX;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mf_trace), sizeof(unsigned long long) * 3 * n) ==
                 hipSuccess ? n : -1;
}
#endif

// form: 4 = FIN_Q threads per panel row (k_sym_finalize_strip), 1 = one thread
// per row with the parts in registers (k_sym_finalize_strip1; bitwise the same
// outputs)
hipError_t launch_sym_finalize_strip(int nc, const SymPanel* d_panels, int npanels,
                                     const PassArgs& pa, const double* rowpart,
                                     const double* colpart, double* partials, int form,
                                     hipStream_t st) {
  // the partials with the default cache policy: nontemporal loads measured
  // 0.5-3 % slower (profiles/r03/s4/fin_nt_ab.jsonl; they were just written)
  if (npanels <= 0) return hipSuccess;   // a block group without packed panels
  if (form != 1 && form != 4) return hipErrorInvalidValue;
  const bool one = form == 1;
#define FIN_CASE(N)                                                                        \
  case N:                                                                                  \
    if (one)                                                                               \
      hipLaunchKernelGGL(k_sym_finalize_strip1<N>, dim3(npanels), dim3(256), 0, st, d_panels, \
                         pa, rowpart, colpart, partials);                                  \
    else                                                                                   \
      hipLaunchKernelGGL(k_sym_finalize_strip<N>, dim3(npanels), dim3(256 * FIN_Q), 0, st, \
                         d_panels, pa, rowpart, colpart, partials);                        \
    break;
  switch (nc) {
    FIN_CASE(1) FIN_CASE(2) FIN_CASE(3) FIN_CASE(4) FIN_CASE(5) FIN_CASE(6) FIN_CASE(7) FIN_CASE(8)
    FIN_CASE(9) FIN_CASE(10) FIN_CASE(11) FIN_CASE(12) FIN_CASE(13) FIN_CASE(14) FIN_CASE(15)
    FIN_CASE(16)
    default: return hipErrorInvalidValue;
  }
#undef FIN_CASE
  return hipGetLastError();
}

}  // namespace sgv
