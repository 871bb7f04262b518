// The kernel form of an LD pass: pass_form decides, from a plan's shape, the
// column count, sgv_set_mfma_min and the seven pass switches, every value that
// selects a kernel instance or a launch argument.  Host arithmetic only (no
// device code, no environment): ld_pass (ldplan.hip) executes the form,
// sgv_ld_pass_form reports it, sgv_pass_form_model is this file on the
// caller's values.
#include "pass_form.h"

#include <cstdint>

#include "sgvamp_hip.h"

namespace sgv {

static_assert(PK_NONE == SGV_KIND_NONE && PK_VALU == SGV_KIND_VALU && PK_STRIP4 == SGV_KIND_STRIP4 &&
                  PK_PAIR == SGV_KIND_PAIR && PK_WIDE == SGV_KIND_WIDE &&
                  PK_STRIP16 == SGV_KIND_STRIP16 && PK_WALK == SGV_KIND_WALK &&
                  PK_FACTOR == SGV_KIND_FACTOR,
              "the header names the kinds");

// Band walks of up to 8 columns (two 4x4x4 column groups; 9-16 columns stay on
// the strips' 16x16x4 kernel): at M = 1e6, bw = 1,000 1.68 / 1.71 / 1.99 ms at
// 3 / 4 / 8 columns against the strips' 1.87 / 1.92 / 2.12
// (profiles/r05/walk_ab/wvs_a_ab.jsonl).
// SGV_BAND_WALK=0: the strips for every band pass (the walks-vs-strips A/B of
// tools/gpu_walk_vs_strips.sh), and a plan built under it has no walk tables.
// An f32 band matrix (sgv_set_ld_precision 32) stays on the 512-column strips at
// every column count: the walks' float instances measured 1.27-1.33x the strips'
// time at 3-4 columns and 1.26-1.31x at 5-8 (M = 1e6, bw = 1,000 and 500, one
// box, alternating: profiles/ld_f32_walk/ldpass_band_ab.jsonl) --
// with half the bytes the walk is bound by its one workgroup's tile, chain and
// hand-off work per sub-tile, which the strips spread over two workgroups per CU.
// SGV_F32_WALK=1: an f32 band-only matrix takes the walks at 3-8 columns,
// whatever sgv_set_mfma_min says (1-2 and 9-16 columns stay on the strips) --
// the arm of that A/B, and how the tests reach the float instances.
bool plan_wants_walks(int bits, const PassSwitches& sw) {
  return sw.band_walk != 0 && (bits != 32 || sw.f32_walk == 1);
}
static bool walk_pass(const PlanShape& ps, int nc, const PassSwitches& sw) {
  return ps.walks && nc <= 8 && sw.band_walk != 0 &&
         (ps.bits != 32 || (nc >= WALK_F32_MIN_NC && sw.f32_walk == 1));
}

// SGV_MF_WIDE_IDLE=0: the idle waves of a ragged chunk stay and add zeros (the
// A/B of their exit)
bool plan_wide_idle(const PassSwitches& sw) { return sw.mf_wide_idle != 0; }

// SGV_MF_PAIR=0 / 1 forces the pair kernel on none / every 3-8-column pass of
// the plan (mfma_pair_choice)
int plan_pair_forced(const PassSwitches& sw) {
  return sw.mf_pair < 0 ? -1 : sw.mf_pair == 1 ? 2 : 0;
}

// Which passes take the wide strips on dense-triangle blocks: every 3-8-column
// pass (one box, parent and this build alternating three times,
// profiles/r07/ldpass_ab.jsonl: 64 x 15,625 at 4 columns -2.1 % per pass, the
// 8-block share -1.5 %; the north star's bench line +2.3 % it/s).
// SGV_MF_WIDE=0 / 1: none / every 3-8-column pass; a forced SGV_MF_PAIR keeps
// the 512-column forms it selects between.  A function of the column count alone.
static bool wide_pass(int nc, const PassSwitches& sw) {
  if (nc < 3 || nc > 8) return false;
  if (sw.mf_wide >= 0) return sw.mf_wide == 1;
  return sw.mf_pair < 0;
}

// The 512-column strips a set runs at nc columns.  The pair kernel: the plan's
// choice (ldplan.hip mfma_pair_choice; bitwise the same products) -- 1: by the
// launch-tail model (a short launch: the 8-block share of the north star), 2
// (forced, SGV_MF_PAIR=1): every launch.  Since the column operands are loaded
// once per row group the model's choice holds at 5-8 columns too: the 8-block
// share -2...-8 %, 4 x 25,000 -2.6 % per 8-column pass; launches it does not
// pick run +1.4...+9 % with the pair form (profiles/r06/pair58_*.jsonl).
// There is no float pair form and no ragged one.
static int strip_kind(int bits, bool ragged, int pair, int nc) {
  if (nc > 8) return PK_STRIP16;
  return bits == 64 && !ragged && pair >= 1 ? PK_PAIR : PK_STRIP4;
}

// SGV_FIN_FORM: the strip finalize's form -- 4 = FIN_Q threads per panel row
// (k_sym_finalize_strip), 1 = one thread per row with the parts in registers
// (k_sym_finalize_strip1; bitwise the same outputs); default: 1 for band plans at
// up to 8 columns (M = 1e6, bw = 1,000: 2.126-2.134 vs 2.156 ms per pass), 4
// otherwise (dense 64 x 15,625 at 8 columns: 12.13 vs 11.97-12.01 ms; 16 columns
// even; profiles/r04/fin_*.jsonl)
static int fin_form(bool ragged, int nc, const PassSwitches& sw) {
  return sw.fin_form > 0 ? sw.fin_form : (ragged && nc <= 8) ? 1 : 4;
}

PassForm pass_form(const PlanShape& ps, int nc, int mfma_min, const PassSwitches& sw) {
  PassForm f;
  f.dense = ps.dense;
  if (!ps.packed) return f;
  // an f32 matrix: every column count on MFMA, whatever mfma_min says (its plan
  // holds no wide strips, and walks only for the SGV_F32_WALK A/B)
  const bool f32 = ps.bits == 32;
  if (!f32 && !(mfma_min > 0 && nc >= mfma_min)) {
    f.kind = PK_VALU;
    f.valu_class = sym_class(nc);
    return f;
  }
  f.pk_width = nc > 8 ? 16 : nc <= 4 ? 4 : 8;
  // 5-8-column passes read Pk PAIRED (k_pack), strips and walks.  Bitwise the
  // same products; one box, alternating: the 8-block share -0.6...-1.8 % per
  // pass, 64 blocks even to -0.4 % (profiles/r06/pkpair_ab.jsonl,
  // pkpair_bench.jsonl)
  f.pk_paired = nc > 4 && nc <= 8;
  // SGV_F32_FORM: the float kernels' load form -- 1 = 8 B per lane (bitwise the
  // f64 strips on the widened matrix), 2 = 16 B per lane (frag_col)
  const bool walk = walk_pass(ps, nc, sw);
  f.load_form = !f32 ? 1 : sw.f32_form > 0 ? sw.f32_form
                     : walk ? WALK_F32_FORM_DEFAULT : F32_FORM_DEFAULT;
  if (walk) {
    f.kind = PK_WALK;
    return f;
  }
  if (!f32 && ps.wide && wide_pass(nc, sw)) {
    f.kind = PK_WIDE;
    f.idle_exit = ps.wide_idle;
    f.side = ps.wide_ngrp > 1;
    if (ps.rest) {   // the plan's other blocks: 512-column strips behind the wide ones
      f.rest_kind = strip_kind(ps.bits, ps.rest_ragged, ps.rest_pair, nc);
      f.fin_form = fin_form(ps.rest_ragged, nc, sw);
      f.rest_side = ps.rest_ngrp > 1;
    }
    return f;
  }
  f.kind = strip_kind(ps.bits, ps.ragged, ps.pair, nc);
  f.mfma16 = f.kind == PK_STRIP16;
  f.fin_form = fin_form(ps.ragged, nc, sw);
  f.side = ps.ngrp > 1;
  return f;
}

void pass_form_ints(const PassForm& f, int32_t* form, int cap) {
  const int32_t v[SGV_PF_N] = {f.kind, f.valu_class, f.rest_kind, f.load_form, f.fin_form,
                               f.pk_width, f.pk_paired, f.dense, f.side, f.rest_side, f.mfma16,
                               f.idle_exit};
  for (int i = 0; i < cap && i < SGV_PF_N; ++i) form[i] = v[i];
}

}  // namespace sgv

extern "C" int sgv_pass_form_model(const int32_t* shape, const int32_t* switches, int mfma_min,
                                   int ncol, int32_t* form, int cap) {
  using namespace sgv;
  if (!shape || !switches || !form || cap < 0 || ncol < 1 || ncol > 16) return SGV_ERR_ARG;
  if (shape[SGV_PS_BITS] != 64 && shape[SGV_PS_BITS] != 32) return SGV_ERR_ARG;
  PlanShape ps;
  ps.bits = shape[SGV_PS_BITS];
  ps.dense = shape[SGV_PS_DENSE] != 0;
  ps.packed = shape[SGV_PS_PACKED] != 0;
  ps.walks = shape[SGV_PS_WALKS] != 0;
  ps.wide = shape[SGV_PS_WIDE] != 0;
  ps.rest = shape[SGV_PS_REST] != 0;
  ps.ragged = shape[SGV_PS_RAGGED] != 0;
  ps.pair = shape[SGV_PS_PAIR];
  ps.rest_ragged = shape[SGV_PS_REST_RAGGED] != 0;
  ps.rest_pair = shape[SGV_PS_REST_PAIR];
  ps.wide_idle = shape[SGV_PS_WIDE_IDLE] != 0;
  ps.ngrp = shape[SGV_PS_NGRP];
  ps.wide_ngrp = shape[SGV_PS_WIDE_NGRP];
  ps.rest_ngrp = shape[SGV_PS_REST_NGRP];
  PassSwitches sw;
  sw.band_walk = switches[SGV_SW_BAND_WALK];
  sw.f32_walk = switches[SGV_SW_F32_WALK];
  sw.mf_wide = switches[SGV_SW_MF_WIDE];
  sw.mf_pair = switches[SGV_SW_MF_PAIR];
  sw.mf_wide_idle = switches[SGV_SW_MF_WIDE_IDLE];
  sw.f32_form = switches[SGV_SW_F32_FORM];
  sw.fin_form = switches[SGV_SW_FIN_FORM];
  // a value the reader would not recognise is not a switch setting
  if ((sw.band_walk != -1 && sw.band_walk != 0) || (sw.f32_walk != -1 && sw.f32_walk != 1) ||
      sw.mf_wide < -1 || sw.mf_wide > 1 || sw.mf_pair < -1 || sw.mf_pair > 1 ||
      (sw.mf_wide_idle != -1 && sw.mf_wide_idle != 0) ||
      (sw.f32_form != -1 && sw.f32_form != 1 && sw.f32_form != 2) ||
      (sw.fin_form != -1 && sw.fin_form != 1 && sw.fin_form != 4))
    return SGV_ERR_ARG;
  pass_form_ints(pass_form(ps, ncol, mfma_min, sw), form, cap);
  return SGV_OK;
}
