// The wave machinery the strip MFMA kernels share (sym_mfma.hip: k_sym_mfma,
// k_sym_mfma_pair, k_sym_mfma_wide), each mechanism defined once:
// the lane decomposition, the Pk operand loads, the branch-free fragment load,
// the prefetch ring, the swizzled LDS tile, the MFMA blocks with the deferred
// row/column interleave, the DPP block reduction and the partial stores.  What a
// kernel keeps of its own (how waves share a chunk, where row sums meet) is in
// sym_mfma.hip above that kernel.  k_sym_mfma16 takes the element types, frag_col
// and lds_order from here and keeps its own loads and ring (see there).
#pragma once
#include "common.h"

#include <type_traits>

namespace sgv {

__device__ __forceinline__ double mfma4(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// wave-local LDS ordering point: lanes of one wave exchange data through the
// tile.  The LDS executes a wave's DS instructions in order, so the write ->
// read (and read -> next write) order only has to survive compilation: a
// wavefront-scope fence, which emits no wait (an inline-asm lgkmcnt(0) would
// make the compiler drain vmcnt as well, stalling on the prefetched loads).
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// spin until the workgroup-scope LDS counter reaches v; ORDER is the load's
// memory order (the hand-off rings of the pair and wide kernels differ in it)
template <int ORDER>
__device__ __forceinline__ void lds_wait_ge(int* ctr, int v) {
  while (__hip_atomic_load(ctr, ORDER, __HIP_MEMORY_SCOPE_WORKGROUP) < v)
    __builtin_amdgcn_s_sleep(1);
}

// Stored element type T of the strip kernels' panels (k_sym_mfma, k_sym_mfma16;
// sgv_set_ld_precision).  A fragment load is two consecutive columns of one row
// per lane: 16 B of an f64 panel, 8 B of an f32 one, for the same 16 x 32
// sub-tile in the same step order.  The prefetch ring keeps them as loaded (an
// f32 ring is half the registers); the step that takes a fragment widens it to
// f64 (v_cvt_f64_f32, exact) ahead of the LDS tile, and everything from there on
// -- tile, MFMA chains, row and column partials -- is one text for both types.
// So every chain of such a float instance (load form 1) sees the operands, in the
// order, that the double instance sees on the widened matrix: its products are
// bitwise equal.  Load form 2 (below) is the one an f32 matrix runs by default.
typedef float f2 __attribute__((ext_vector_type(2)));
template <class T>
struct Frag;
template <>
struct Frag<double> {
  typedef d2 raw;
  static __device__ __forceinline__ d2 widen(d2 v) { return v; }
};
template <>
struct Frag<float> {
  typedef f2 raw;
  static __device__ __forceinline__ d2 widen(f2 v) { return d2{(double)v.x, (double)v.y}; }
};
// Load form LF = 2 (float panels only): 16 B per lane, a float4 of 4 consecutive
// columns, one load per 64-column super-step feeding two 32-column steps -- half
// the load instructions per element.  Sub-step e' of super-step S is step t = 2 S
// + e', and its pair index p (the lane's place in the fragment, the tile and the
// column accumulators) stands for chunk columns 64 S + 4 p + 2 e', + 1 instead
// of 32 t + 2 p, + 1 (frag_col): the row-part operands, the loads and the column
// stores take their columns from it, nothing else changes.  A row's terms are
// then added in another fixed order: not bitwise the LF = 1 sums, still a function
// of the block alone.
typedef float f4 __attribute__((ext_vector_type(4)));
template <int LF>
__device__ __forceinline__ constexpr int frag_col(int t, int p) {
  return LF == 2 ? 64 * (t >> 1) + 4 * p + 2 * (t & 1) : 32 * t + 2 * p;
}
// 32-column steps with a column below nrem (columns left from the wave's first)
template <int LF>
__device__ __forceinline__ int steps_upto(int nrem) {
  return LF == 2 ? 2 * ((nrem + 63) / 64) : (nrem + 31) / 32;
}

// the row group after the current one: this panel's g + 1, or the next panel's
// first (the prefetch crosses panel boundaries through selects); past the
// strip's last row group the cache-resident Pk with stride 0 (load_cf)
struct NextGroup {
  uint64_t b;    // panel base (pbase)
  int64_t w;     // row stride
  int H, nc, g, r0;
  bool z;        // its column-part B operands are 0 (diagonal block)
};

// One wave's view of its strip.  NG: 4-column groups of right-hand sides; PP:
// Pk in k_pack's PAIRED layout (NG = 2), so a lane's two column groups (columns
// n4 and 4 + n4) of one Pk row are one 16-B load: half the P-operand load
// instructions through the texture-address unit per row group.  T, LF: stored
// type and load form (above).  RAG: some item of the strip stops short of the
// strip's widest (band plans).
// SWZ (NG = 2): column-part B operands without the 4x replication over the
// MFMA blocks: blocks 0-1 take a row group's 4-row sets in the order 0 1 2 3,
// blocks 2-3 in the order 2 3 0 1 (fragment a of a lane is row set a ^ (bq &
// 2)), so one Pk load per row group (lane: row set bq) holds every set a block
// needs and ds_swizzle hands each lane its set for fragment a (swz_quad); the
// R fragment loads stay whole 128-B lines.  One box, alternating: the north
// star -0.4...-0.8 % per pass, the 8-block share -1.4 %; at NG = 1 (8-B
// operands) even to +0.4 %, so not there (profiles/r06/mf_sw_*.jsonl)
template <int NG, bool PP, class T = double, int LF = 1, bool RAG = false, bool SWZ = (NG == 2)>
struct StripWave {
  static_assert(!PP || NG == 2, "paired Pk rows: two column groups");
  static constexpr bool W4 = LF == 2;   // 16-B loads of float panels (frag_col)
  static_assert(!W4 || sizeof(T) == 4, "LF = 2: float panels");
  typedef T elem;
  typedef typename std::conditional<W4, f4, typename Frag<T>::raw>::type RV;   // a fragment as loaded
  static constexpr int NB = SWZ ? 1 : 4;   // column-part operand sets a lane loads per row group
  static constexpr int RW = 4 * NG;        // row-sum stride of the per-wave row buffers

  int lo, hi, bq, n4, pc;
  const double* pkb;   // Pk of this block (block-relative index)
  int pks;             // Pk row stride (k_pack)
  int c0, ncc;         // the strip's chunk: first column, widest item
  int cw0;             // first chunk column of this wave
  bool dhalf;          // wave inside a diagonal panel's diagonal block

  __device__ __forceinline__ StripWave(int lane, const double* pkb_, int pks_, int c0_, int ncc_,
                                       int cw0_, bool dhalf_)
      : lo(lane & 15), hi(lane >> 4), bq((lane >> 2) & 3), n4(lane & 3),
        pc(hi + 4 * bq),   // this lane's column pair in a fragment
        pkb(pkb_), pks(pks_), c0(c0_), ncc(ncc_), cw0(cw0_), dhalf(dhalf_) {}

  // A wave's 32-column steps at or past the chunk's last column (the ragged
  // last chunk of a panel: 4 % of the north star's steps) take no LDS or MFMA
  // work -- their row-part B operands are 0 and their column sums are never
  // read, so every kept sum is bitwise the same; nor do the column MFMAs of the
  // diagonal-block waves of a diagonal panel (B = 0 there).  The loads stay, so
  // the load count is the same on every path.
  // The wave's steps with a column below nlim.
  __device__ __forceinline__ int steps_to(int nlim) const {
    return max(0, steps_upto<LF>(nlim - cw0));
  }

  // one Pk row's values of this lane: column 4 q + n4 for each group q
  __device__ __forceinline__ void ld_prow(int64_t row, double* v) const {
    if constexpr (PP) {
      const d2 x = ldg((const d2*)(pkb + row * pks + 2 * n4));
      v[0] = x.x;
      v[1] = x.y;
    } else {
#pragma unroll
      for (int q = 0; q < NG; ++q) v[q] = ldg(pkb + row * pks + 4 * q + n4);
    }
  }

  // row-part B operands: P at this wave's columns, reused by every row group
  template <int NT>
  __device__ __forceinline__ void load_brow(double (&brow)[NT][2][NG]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int col = cw0 + frag_col<LF>(t, pc) + e;
        double v[NG];
        ld_prow(c0 + (col < ncc ? col : 0), v);
#pragma unroll
        for (int q = 0; q < NG; ++q) brow[t][e][q] = col < ncc ? v[q] : 0.0;
      }
  }

  // fragment loads of step (g, t) of a panel (b0 = its element (r0, c0)), 16 B
  // per lane (8 B of an f32 panel; strides and offsets in elements), branch-free:
  // a row past H clamps (its P is 0), a column past the chunk (RAG: past the
  // item, nci) loads column 0 (finite; it meets a zero B in the row part and is
  // never read from the column part).  The base is an opaque integer: a pointer
  // select is turned back into a branch with one load per side.  Past the
  // strip's last row group the caller passes the cache-resident Pk with stride 0
  // (a dummy fetch: the load count is the same on every path, so the compiler
  // never drains vmcnt(0) at a branch join or the row-group loop head).
  // (LF = 2: t counts super-steps, one float4 of columns 64 t + 4 lo ..)
  __device__ __forceinline__ void load_cf(uint64_t b0, int64_t ws, int H, int nci, int g, int t,
                                          RV* cf) const {
    asm volatile("" : "+s"(b0));
    const int xc = W4 ? cw0 + 64 * t + 4 * lo : cw0 + 32 * t + 2 * lo;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int rB = 16 * g + 4 * (SWZ ? a ^ (bq & 2) : a) + hi;
      const T* row = (const T*)b0 + (int64_t)(rB < H ? rB : H - 1) * ws;
      cf[a] = ldg_nt((const RV*)(row + (xc < (RAG ? nci : ncc) ? xc : 0)));
    }
  }

  // column-part B operands of row group g of a panel (first row r0): P at its
  // rows; zero past H and, for the diagonal panel, in the diagonal-block waves
  // (SWZ: bc[0] = this lane's row set bq, handed to the fragments by hand_bcol)
  __device__ __forceinline__ void load_bcol(int r0, int H, bool zero, int g,
                                            double (&bc)[NB][NG]) const {
#pragma unroll
    for (int a = 0; a < NB; ++a) {
      const int rB = 16 * g + 4 * (SWZ ? bq : a) + hi;
      double v[NG];
      ld_prow(r0 + (rB < H ? rB : 0), v);
#pragma unroll
      for (int q = 0; q < NG; ++q) bc[a][q] = (rB < H && !zero) ? v[q] : 0.0;
    }
  }

  // the loaded operands as fragment a's: SWZ, set a ^ (bq & 2) from the lane of
  // quad a ^ (bq & 2) of this 16-lane row
  __device__ __forceinline__ void hand_bcol(const double (&bcn)[NB][NG],
                                            double (&bcol)[4][NG]) const {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < NG; ++q) bcol[a][q] = SWZ ? swz_quad(bcn[0][q], a) : bcn[SWZ ? 0 : a][q];
  }

  // a panel's element (r0, c0) as load_cf's opaque base
  static __device__ __forceinline__ uint64_t pbase(const SymItem& x) {
    return (uint64_t)((const T*)x.P + (x.c0 - x.r0));
  }

  // is the wave's column-part B zero in the panel whose first row is r0
  __device__ __forceinline__ bool col_zero(int r0) const { return dhalf && r0 == c0; }

  __device__ __forceinline__ NextGroup next_group(int g, int ng, const SymItem& cur, uint64_t curb,
                                                  bool more, const SymItem& nx,
                                                  uint64_t nxb) const {
    const bool same = g + 1 < ng;
    NextGroup n;
    n.b = same ? curb : nxb;
    n.w = same ? cur.w : (more ? nx.w : 0);
    n.H = same ? cur.H : (more ? nx.H : 1);
    n.nc = same ? cur.nc : nx.nc;
    n.g = same ? g + 1 : 0;
    n.r0 = same ? cur.r0 : nx.r0;
    n.z = col_zero(n.r0);
    return n;
  }

  // a band panel's item narrower than the strip: its columns past nci (never
  // loaded: load_cf took column 0) read as zero
  __device__ __forceinline__ void band_zero(int nci, int t, d2* cf) const {
    const int xc = cw0 + frag_col<LF>(t, lo);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      cf[a].x = xc < nci ? cf[a].x : 0.0;
      cf[a].y = xc + 1 < nci ? cf[a].y : 0.0;
    }
  }

  // The per-wave transpose tile of the 4x4x4 kernels: 16 rows x 32 columns, 16-B
  // piece (row r, pair p) at slot 16 r + (p ^ (r & 3)) -- unpadded (4 KiB, so
  // k_sym_mfma's 64 KiB of row sums and the tiles fit two workgroups per CU) and
  // conflict-free both ways: a write's 16-lane quarter covers one row, a
  // row-fragment read's quarter (rows 4q + (l & 3), pairs 4((l >> 2) & 3) + (l
  // >> 4)) 16 distinct slots mod 16.  The row fragment reads go out right
  // behind the writes (a wave's DS operations execute in order); the column
  // MFMAs that follow cover their latency.
  __device__ __forceinline__ void tile_exchange(double* sb, const d2* cf, d2* rf) const {
    lds_order();                                   // previous step's tile reads issued
#pragma unroll
    for (int a = 0; a < 4; ++a)
      *(d2*)(sb + 32 * (4 * (SWZ ? a ^ (bq & 2) : a) + hi) + 2 * (lo ^ hi)) = cf[a];
    lds_order();                                   // tile written
#pragma unroll
    for (int r = 0; r < 4; ++r) rf[r] = *(const d2*)(sb + 32 * (4 * r + n4) + 2 * (pc ^ n4));
  }

  // a row group's row sums: the 4 blocks (lanes differing in bits 2,3; DPP row
  // rotations, fixed order) into a 16 x RW buffer, D row 4r + m (m = hi)
  __device__ __forceinline__ void reduce_blocks(const double (&drow)[4][NG], double* wb) const {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        double v = drow[r][q];
        v = v + row_ror<12>(v);
        v = v + row_ror<8>(v);
        if (bq == 0) wb[(4 * r + hi) * RW + 4 * q + n4] = v;
      }
  }

  // column sums over the strip's panels: D_b[m][n] at lane 16m + 4b + n holds
  // column pair 4b + m = pc, column c = 4q + n.  The wave's whole segment, 16-B
  // stores (columns the finalize never reads: don't care).  out: the strip's
  // colpart slot at column n4, chunk column cw0 + 2 p0 (p = pc - p0 is added
  // here); CW: the slot's width.
  template <int NT, int CW>
  __device__ __forceinline__ void store_colpart(double* out, int p, int ncol,
                                                const double (&dcol)[NT][2][NG]) const {
#pragma unroll
    for (int q = 0; q < NG; ++q)
      if (4 * q + n4 < ncol) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          *(d2*)(out + 4 * q * CW + frag_col<LF>(t, p)) = d2{dcol[t][0][q], dcol[t][1][q]};
      }
  }
};

// The prefetch ring: PD steps (of NT per row group) in flight per wave, kept as
// loaded.  step(t) takes step t's fragments, widened, and issues in their place
// the load of step t + PD of this row group or, past its end, of the next one
// (n), whose column-part operands go out with its first step.
// LF = 2: the ring holds the row group's NT / 2 super-steps; a super-step's
// float4s are taken (and widened) at its first step, and the same super-step of
// the next row group goes out in their place.
template <class SW, int PD, int NT>
struct FragRing {
  static_assert(PD >= 1 && PD <= NT && NT % PD == 0, "prefetch depth divides the steps");
  static_assert(!SW::W4 || (PD == 2 && NT % 2 == 0), "LF = 2: two super-steps");
  static constexpr int RD = SW::W4 ? NT / 2 : PD;   // ring depth (LF = 2: in super-steps, the same bytes)
  typename SW::RV q[RD][4];
  d2 w[SW::W4 ? 2 : 1][4];   // LF = 2: a super-step's two steps, widened

  __device__ __forceinline__ void prime(const SW& sw, uint64_t curb, const SymItem& cur) {
#pragma unroll
    for (int p = 0; p < RD; ++p) sw.load_cf(curb, cur.w, cur.H, cur.nc, 0, p, q[p]);
  }

  template <int NG>
  __device__ __forceinline__ void step(const SW& sw, int t, int g, uint64_t curb,
                                       const SymItem& cur, const NextGroup& n,
                                       double (&bcn)[SW::NB][NG], d2* cf) {
    if constexpr (SW::W4) {
      if ((t & 1) == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const f4 v = q[t >> 1][a];
          w[0][a] = d2{(double)v.x, (double)v.y};
          w[1][a] = d2{(double)v.z, (double)v.w};
        }
        sw.load_cf(n.b, n.w, n.H, n.nc, n.g, t >> 1, q[t >> 1]);
        if (t + PD == NT) sw.load_bcol(n.r0, n.H, n.z, n.g, bcn);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) cf[a] = w[t & 1][a];
    } else {
      const int slot = t % PD;                       // compile-time after unrolling
#pragma unroll
      for (int a = 0; a < 4; ++a) cf[a] = Frag<typename SW::elem>::widen(q[slot][a]);
      // step + PD goes out here, ahead of this step's LDS and MFMA work
      if (t + PD < NT) {
        sw.load_cf(curb, cur.w, cur.H, cur.nc, g, t + PD, q[slot]);
      } else {
        sw.load_cf(n.b, n.w, n.H, n.nc, n.g, t + PD - NT, q[slot]);
        if (t + PD == NT) sw.load_bcol(n.r0, n.H, n.z, n.g, bcn);
      }
    }
  }
};

template <int A, int B>
__device__ __forceinline__ void zero(double (&x)[A][B]) {
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int b = 0; b < B; ++b) x[a][b] = 0.0;
}
template <int A, int B, int C>
__device__ __forceinline__ void zero(double (&x)[A][B][C]) {
#pragma unroll
  for (int a = 0; a < A; ++a) zero(x[a]);
}

// one step's column part, level a: Dcol[pair][c] += R[j][i] P[j][c] over the 4
// rows of fragment a
template <int NG>
__device__ __forceinline__ void col_mfma(d2 cfa, const double (&b)[NG], double (&dc)[2][NG]) {
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    dc[0][q] = mfma4(cfa.x, b[q], dc[0][q]);
    dc[1][q] = mfma4(cfa.y, b[q], dc[1][q]);
  }
}
// one step's row part: x halves of all 4*NG row chains, then the y halves: a
// chain's two MFMAs are 4*NG issues apart instead of back to back (same
// per-chain order)
template <int NG>
__device__ __forceinline__ void row_mfma(const d2* f, const double (&br)[2][NG],
                                         double (&drow)[4][NG]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < NG; ++q) drow[r][q] = mfma4(f[r].x, br[0][q], drow[r][q]);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < NG; ++q) drow[r][q] = mfma4(f[r].y, br[1][q], drow[r][q]);
}
// step t, plain: the column levels (unless their B is zero: colz), then the rows
template <int NG>
__device__ __forceinline__ void mfma_step(bool colz, const d2* cf, const d2* rf, bool rows,
                                          const double (&bcol)[4][NG], const double (&br)[2][NG],
                                          double (&dc)[2][NG], double (&drow)[4][NG]) {
  if (!colz) {
#pragma unroll
    for (int a = 0; a < 4; ++a) col_mfma<NG>(cf[a], bcol[a], dc);
  }
  if (rows) row_mfma<NG>(rf, br, drow);
}
// step t, deferred (DEF): a step's row MFMAs are deferred into the next step and
// interleaved with its column MFMAs, so consecutive MFMAs of one accumulator
// chain sit 8 issues apart instead of 4 (2 at NG = 1); every chain accumulates
// in the same order (bitwise the same sums), the row fragments are
// double-buffered in registers (rf: this step's, rp: the previous step's).
// Column level a of this step, then a quarter of the previous step's row MFMAs
// (x halves of rows 2(a&1), +1 for a < 2, then the y halves); the row group's
// last active step (last) runs its own row MFMAs at once.
template <int NG, int NT>
__device__ __forceinline__ void mfma_step_deferred(int t, bool last, bool colz, const d2* cf,
                                                   const d2* rf, const d2* rp,
                                                   const double (&bcol)[4][NG],
                                                   const double (&brow)[NT][2][NG],
                                                   double (&dc)[2][NG], double (&drow)[4][NG]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (!colz) col_mfma<NG>(cf[a], bcol[a], dc);
    if (t > 0) {
      const int tp = t > 0 ? t - 1 : 0;
#pragma unroll
      for (int r = 2 * (a & 1); r < 2 * (a & 1) + 2; ++r)
#pragma unroll
        for (int q = 0; q < NG; ++q)
          drow[r][q] = mfma4(a < 2 ? rp[r].x : rp[r].y, brow[tp][a < 2 ? 0 : 1][q], drow[r][q]);
    }
  }
  if (last) row_mfma<NG>(rf, brow[t], drow);
}

// a panel's H x ncol row sums out of NSRC per-wave (per-segment) buffers of
// SYM_H x RW: sources in order, contiguous in rowpart (dst); NTHR threads
template <int NSRC, int NTHR, int RW>
__device__ __forceinline__ void panel_rows_out(const double* rows, int H, int ncol, double* dst) {
  const int n = H * ncol;
  for (int i = threadIdx.x; 2 * i < n; i += NTHR) {
    double v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = 2 * i + e < n ? 2 * i + e : 2 * i;
      const int row = k / ncol, cc = k - row * ncol;
      const double* src = rows + row * RW + cc;
      double x = src[0];
#pragma unroll
      for (int w = 1; w < NSRC; ++w) x += src[w * SYM_H * RW];
      v[e] = x;
    }
    if (2 * i + 1 < n)
      *(d2*)(dst + 2 * i) = d2{v[0], v[1]};
    else
      dst[2 * i] = v[0];
  }
}

}  // namespace sgv
