// The float instances of k_band_walk (band_walk.h): the walks of an LD matrix
// stored as f32, the A/B arm SGV_AB=1 SGV_F32_WALK=1 (ldplan.hip).  A
// translation unit of their own, so that the f64 instances of band_walk.hip
// compile as if these did not exist.
#include "band_walk.h"

namespace sgv {

// the form an f32 band matrix walks with: SGV_F32_FORM (A/B, with SGV_AB=1; the
// strips' switch) 1 = 8 B per lane, the bitwise pin; 2 = 16 B per lane, 2-3 %
// faster on every line of the A/B (profiles/ld_f32_walk/ldpass_band_ab.jsonl);
// read per launch (a getenv)
constexpr int WALK_F32_FORM_DEFAULT = 2;
static int walk_f32_form() {
  const char* e = ab_env("SGV_F32_FORM");
  return (e && (e[0] == '1' || e[0] == '2')) ? e[0] - '0' : WALK_F32_FORM_DEFAULT;
}

void launch_walks_f32(int nc, const SymWalk* d_walks, int nwalks, const SymPanel* d_panels,
                      const SymItem* d_items, const double* d_pk, int pks, int64_t pk_rows,
                      const PassArgs& pa, double* headbuf, double* carrybuf, double* partials,
                      hipStream_t st) {
  const int form = walk_f32_form();
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
