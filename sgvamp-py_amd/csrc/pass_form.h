// Which kernel form an LD pass takes (pass_form.cpp): one decision over plain
// values -- no context, no HIP call, no environment -- so it runs on a machine
// without a device (sgv_pass_form_model, tests/test_pass_form.py).  ldplan.hip
// reads the switches (read_pass_switches), ld_pass launches what the form says,
// and sgv_ld_pass_form reports it.
#pragma once
#include <cstdint>

namespace sgv {

// What the decision needs from an LdPlan, and nothing else.  The plan keeps what
// it was built under: pair (mfma_pair_choice), wide_idle and the presence of the
// walk tables.
struct PlanShape {
  int bits = 64;               // element type of the packed blocks (64 / 32)
  bool dense = false;          // dense row groups
  bool packed = false;         // packed panels
  bool walks = false;          // walk tables
  bool wide = false;           // the wide set has strips
  bool rest = false;           // the rest set has strips
  bool ragged = false;         // s512
  int pair = 0;
  bool rest_ragged = false;    // rest
  int rest_pair = 0;
  bool wide_idle = true;
  int ngrp = 1, wide_ngrp = 1, rest_ngrp = 1;   // block groups of s512 / wide / rest
};

// The seven pass switches as read_pass_switches found
// them: -1 unset, ignored without SGV_AB=1 or not one of the switch's values
struct PassSwitches {
  int band_walk = -1;      // SGV_BAND_WALK: 0
  int f32_walk = -1;       // SGV_F32_WALK: 1
  int mf_wide = -1;        // SGV_MF_WIDE: 0 / 1
  int mf_pair = -1;        // SGV_MF_PAIR: 0 / 1
  int mf_wide_idle = -1;   // SGV_MF_WIDE_IDLE: 0
  int f32_form = -1;       // SGV_F32_FORM: 1 / 2
  int fin_form = -1;       // SGV_FIN_FORM: 1 / 4
};

// the packed kinds: the values of SGV_PF_KIND and SGV_PF_REST_KIND (sgvamp_hip.h)
enum PackedKind {
  PK_NONE = 0,      // no packed panels
  PK_VALU = 1,      // the packed VALU pass in chunk class valu_class
  PK_STRIP4 = 2,    // 4-wave 512-column strips (k_sym_mfma)
  PK_PAIR = 3,      // wave-pair 512-column strips (k_sym_mfma_pair)
  PK_WIDE = 4,      // 1,024-column strips (k_sym_mfma_wide), `rest` behind them
  PK_STRIP16 = 5,   // 16x16x4 strips at 9-16 columns (k_sym_mfma16)
  PK_WALK = 6,      // band walks (k_band_walk)
  PK_FACTOR = 7     // a factor matrix (geno_factor.hip): the plan's own predicate in ldplan.hip,
                    // never pass_form's answer -- no PlanShape describes it
};

// Everything that selects a kernel instance or a launch argument of one pass
struct PassForm {
  int kind = PK_NONE;
  int valu_class = -1;       // PK_VALU: chunk-width class (CW = 1024 >> class)
  int rest_kind = PK_NONE;   // PK_WIDE: the rest set's strips (PK_STRIP4 / PK_PAIR)
  int load_form = 0;         // MFMA kinds: 1 = 8 B per lane (every f64 matrix), 2 = 16 B
  int fin_form = 0;          // the strip finalize that runs (s512's, or rest's): 1 / 4
  int pk_width = 0;          // doubles per Pk row: 4 / 8 / 16
  bool pk_paired = false;
  bool dense = false;        // the dense row-group kernel runs
  bool side = false;         // the set's finalizes on the side stream (s512, or wide)
  bool rest_side = false;    // PK_WIDE: the rest set's
  bool mfma16 = false;       // a 9-16-column MFMA pass (sgv_timers t[7..9])
  bool idle_exit = false;    // PK_WIDE: idle waves leave at the start
};

// the load form an f32 matrix's strips run: 2, faster than 1 on every line of
// the A/B (64 x 15,625 -1...-5 % per pass, 8 x 15,625 -3...-9 %: DESIGN.md 4.6,
// profiles/ld_f32/ldpass_ab.jsonl); 1 stays compiled as the bitwise pin
constexpr int F32_FORM_DEFAULT = 2;
// the form an f32 band matrix walks with: 1 = 8 B per lane, the bitwise pin; 2 =
// 16 B per lane, 2-3 % faster on every line of the A/B
// (profiles/ld_f32_walk/ldpass_band_ab.jsonl)
constexpr int WALK_F32_FORM_DEFAULT = 2;
// the fewest columns an f32 matrix walks with (SGV_F32_WALK=1)
constexpr int WALK_F32_MIN_NC = 3;

// chunk-width class of the packed VALU pass for nc columns (CW = 1024 >> cls)
static inline int sym_class(int nc) { return nc <= 2 ? 0 : nc <= 4 ? 1 : nc <= 8 ? 2 : 3; }

// the form a pass of nc columns (1..16) over a plan of this shape takes
PassForm pass_form(const PlanShape& ps, int nc, int mfma_min, const PassSwitches& sw);

// the form as the ints of sgv_ld_pass_form (SGV_PF_*, sgvamp_hip.h): min(cap, SGV_PF_N) values
void pass_form_ints(const PassForm& f, int32_t* form, int cap);

// What a plan is built under (ensure_plan): whether it makes walk tables for a
// band matrix of this element type, whether the wide kernel's idle waves leave,
// and the forced pair choice (-1: by the launch-tail model, 0 none, 2 every pass)
bool plan_wants_walks(int bits, const PassSwitches& sw);
bool plan_wide_idle(const PassSwitches& sw);
int plan_pair_forced(const PassSwitches& sw);

}  // namespace sgv
