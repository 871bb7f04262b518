// The float instances of k_band_walk (band_walk.h): the walks of an LD matrix
// stored as f32, the A/B arm SGV_AB=1 SGV_F32_WALK=1 (pass_form.cpp).  A
// translation unit of their own, so that the f64 instances of band_walk.hip
// compile as if these did not exist.
#include "band_walk.h"

namespace sgv {

// form: the load form (pass_form.cpp), 1 = 8 B per lane, 2 = 16 B per lane
void launch_walks_f32(int nc, const SymWalk* d_walks, int nwalks, const SymPanel* d_panels,
                      const SymItem* d_items, const double* d_pk, int pks, int64_t pk_rows,
                      const PassArgs& pa, double* headbuf, double* carrybuf, double* partials,
                      int form, hipStream_t st) {
#define SGV_WALK(NG)                                                                           \
  (form == 2 ? launch_walk<NG, float, 2> : launch_walk<NG, float, 1>)(                         \
      d_walks, nwalks, d_panels, d_items, d_pk, pks, pk_rows, pa, nc, headbuf, carrybuf, partials, st)
  if (nc <= 4)
    SGV_WALK(1);
  else
    SGV_WALK(2);
#undef SGV_WALK
}

}  // namespace sgv
