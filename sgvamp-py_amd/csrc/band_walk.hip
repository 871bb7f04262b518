// The band walks' launches: k_band_walk (band_walk.h) on f64 panels, the head
// panels' k_walk_fin, and the hand-over of float panels to band_walk_f32.hip.
#include "band_walk.h"

namespace sgv {

// Head panels of the walks: y = the walk's partial + the previous walk's carry
// (+ the coupling sum), then the epilogue and the panel's partial dots -- as
// k_band_walk's own epilogue
template <int RW>
__global__ __launch_bounds__(256) void k_walk_fin(const WalkFin* __restrict__ fins,
                                                  const SymPanel* __restrict__ panels, PassArgs pa,
                                                  int ncol, const double* __restrict__ headbuf,
                                                  const double* __restrict__ carrybuf,
                                                  double* __restrict__ partials) {
  __shared__ double s_w[4 * RW];
  const WalkFin f = fins[blockIdx.x];
  if (pa.run && !ldg(pa.run)) return;
  const SymPanel pn = panels[f.panel];
  const int t = threadIdx.x;
  const double* hb = headbuf + ((int64_t)f.hslot * SYM_H + t) * ncol;
  const double* cb = carrybuf + ((int64_t)f.cslot * SYM_H + t) * ncol;
  double y[RW];
#pragma unroll
  for (int c = 0; c < RW; ++c) y[c] = c < ncol ? hb[c] + cb[c] : 0.0;
  walk_epilogue<RW, 1>(pn, pa, ncol, y, s_w);
  __syncthreads();
  if (t < ncol)
    partials[(int64_t)pn.part * ncol + t] =
        ((s_w[0 * RW + t] + s_w[1 * RW + t]) + s_w[2 * RW + t]) + s_w[3 * RW + t];
}

// bits: the stored type of the items' panels (LdPlan::bits); form: the float
// instances' load form; pks: Pk's row width, 4 up to 4 columns and 8 above
hipError_t launch_band_walk(int nc, const SymWalk* d_walks, int nwalks, const SymPanel* d_panels,
                            const SymItem* d_items, const double* d_pk, int pks, int64_t pk_rows,
                            const PassArgs& pa,
                            double* headbuf, double* carrybuf, const WalkFin* d_fins, int nfins,
                            double* partials, int bits, int form, hipStream_t st) {
  if (nc < 1 || nc > 8) return hipErrorInvalidValue;
  if (bits != 64 && bits != 32) return hipErrorInvalidValue;
  if (pks != (nc <= 4 ? 4 : 8)) return hipErrorInvalidValue;   // the instances' column groups
  if (nwalks > 0) {
    if (bits == 32)
      launch_walks_f32(nc, d_walks, nwalks, d_panels, d_items, d_pk, pks, pk_rows, pa, headbuf,
                       carrybuf, partials, form, st);
    else if (nc <= 4)
      launch_walk<1, double, 1>(d_walks, nwalks, d_panels, d_items, d_pk, pks, pk_rows, pa, nc,
                                headbuf, carrybuf, partials, st);
    else
      launch_walk<2, double, 1>(d_walks, nwalks, d_panels, d_items, d_pk, pks, pk_rows, pa, nc,
                                headbuf, carrybuf, partials, st);
  }
  if (nfins > 0) {
    if (nc <= 4)
      hipLaunchKernelGGL(k_walk_fin<4>, dim3(nfins), dim3(256), 0, st, d_fins, d_panels, pa, nc,
                         headbuf, carrybuf, partials);
    else
      hipLaunchKernelGGL(k_walk_fin<8>, dim3(nfins), dim3(256), 0, st, d_fins, d_panels, pa, nc,
                         headbuf, carrybuf, partials);
  }
  return hipGetLastError();
}

}  // namespace sgv
