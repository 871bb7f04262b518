// Host-side sanitizer run of the library's host-only code (tests/test_asan_host.py):
// csrc/hybrd.cpp (the fsolve restatement), csrc/probes.cpp (the MT19937
// binomial probe stream) and csrc/pass_form.cpp (the LD pass's form decision)
// built with -fsanitize=address,undefined and driven on a few systems, on
// split / whole probe draws and over the whole product of plan shapes, column
// counts and switch settings.  GPU code is out of reach of
// the sanitizers on this pool; this covers the host code the GPU tests call.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pass_form.h"
#include "sgvamp_hip.h"

extern "C" int sgv_probe_draw(uint32_t* key, int32_t* pos, int64_t n, int64_t lo, int64_t hi,
                              int8_t* out);

static int rosen(void*, int n, const double* x, double* f) {
  (void)n;
  f[0] = 10.0 * (x[1] - x[0] * x[0]);
  f[1] = 1.0 - x[0];
  return 0;
}
static int trig(void*, int n, const double* x, double* f) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += std::cos(x[i]);
  for (int i = 0; i < n; ++i) f[i] = n - s + (i + 1) * (1.0 - std::cos(x[i])) - std::sin(x[i]);
  return 0;
}
static int rootless(void*, int n, const double* x, double* f) {
  for (int i = 0; i < n; ++i) f[i] = x[i] * x[i] + 1.0;
  return 0;
}
static int stop_early(void* u, int n, const double* x, double* f) {
  int* calls = (int*)u;
  if (++*calls > 3) return -1;
  return trig(nullptr, n, x, f);
}

static void seed_mt(uint32_t* key, uint32_t s) {   // the standard MT19937 init_genrand
  key[0] = s;
  for (int i = 1; i < 624; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + i;
}

int main() {
  int bad = 0;
  {
    double x[2] = {-1.2, 1.0}, f[2];
    int nfev = 0;
    const int ier = sgv_fsolve(2, rosen, nullptr, x, f, &nfev);
    std::printf("rosenbrock ier=%d nfev=%d x=(%.6f, %.6f)\n", ier, nfev, x[0], x[1]);
    bad += ier != 1 || std::fabs(x[0] - 1.0) > 1e-8;
  }
  for (int n : {1, 3, 10, 40}) {
    std::vector<double> x(n, 1.0 / n), f(n);
    int nfev = 0;
    const int ier = sgv_fsolve(n, trig, nullptr, x.data(), f.data(), &nfev);
    std::printf("trig n=%d ier=%d nfev=%d\n", n, ier, nfev);
    bad += ier < 1 || ier > 5;
  }
  {
    double x[3] = {1.0, 2.0, 3.0}, f[3];
    int nfev = 0;
    const int ier = sgv_fsolve(3, rootless, nullptr, x, f, &nfev);
    std::printf("rootless ier=%d nfev=%d\n", ier, nfev);
    bad += ier == 1;
  }
  {
    double x[4] = {0.1, 0.2, 0.3, 0.4}, f[4];
    int nfev = 0, calls = 0;
    const int ier = sgv_fsolve(4, stop_early, &calls, x, f, &nfev);
    std::printf("stopped ier=%d nfev=%d\n", ier, nfev);
  }
  // probe stream: one call draws samples [lo, hi) of a stream of n (2 words
  // each) and leaves the key 2n words on; the pieces [0, a), [a, b), [b, n)
  // drawn from copies of one state equal the whole draw, every state after
  // equals the whole draw's, at even and odd stream positions
  const int64_t n = 5000;
  for (int32_t p0 : {624, 0, 1, 17}) {
    for (int64_t a : {0, 1, 311, 624, 1247}) {
      for (int64_t b : {a, a + 1, a + 700, n}) {
        if (b > n) continue;
        uint32_t k0[624];
        seed_mt(k0, 12345u);
        std::vector<int8_t> whole(n), parts(n);
        uint32_t kw[624];
        std::memcpy(kw, k0, sizeof k0);
        int32_t pw = p0;
        bad += sgv_probe_draw(kw, &pw, n, 0, n, whole.data()) != 0;
        const int64_t cut[4] = {0, a, b, n};
        for (int s = 0; s < 3; ++s) {
          uint32_t k[624];
          std::memcpy(k, k0, sizeof k0);
          int32_t p = p0;
          bad += sgv_probe_draw(k, &p, n, cut[s], cut[s + 1], parts.data() + cut[s]) != 0;
          bad += p != pw || std::memcmp(k, kw, sizeof k) != 0;
        }
        bad += std::memcmp(whole.data(), parts.data(), n) != 0;
      }
    }
  }
  {   // argument checks
    uint32_t k[624];
    seed_mt(k, 1u);
    int32_t p = 624;
    int8_t o[4];
    bad += sgv_probe_draw(k, &p, 4, 3, 2, o) == 0;
    bad += sgv_probe_draw(k, &p, 4, 0, 5, o) == 0;
    bad += sgv_probe_draw(nullptr, &p, 4, 0, 4, o) == 0;
  }
  {   // pass_form over the product tests/test_pass_form.py sweeps, through the model's ints:
      // every form inside its ranges, the direct call and the model agree
    const int sv[SGV_SW_N][3] = {{-1, 0, 0}, {-1, 1, 1}, {-1, 0, 1}, {-1, 0, 1},
                                 {-1, 0, 0}, {-1, 1, 2}, {-1, 1, 4}};
    const int sn[SGV_SW_N] = {2, 2, 3, 3, 2, 3, 3};
    long n_forms = 0;
    for (int bits : {64, 32})
      for (int mm : {0, 1, 3, 9})
        for (int nc = 1; nc <= 16; ++nc)
          for (int shape_bits = 0; shape_bits < 16 * 3; ++shape_bits) {
            int32_t sh[SGV_PS_N] = {};
            sh[SGV_PS_BITS] = bits;
            sh[SGV_PS_PACKED] = 1;
            sh[SGV_PS_WALKS] = shape_bits & 1;
            sh[SGV_PS_WIDE] = shape_bits >> 1 & 1;
            sh[SGV_PS_REST] = shape_bits >> 2 & 1;
            sh[SGV_PS_RAGGED] = sh[SGV_PS_REST_RAGGED] = shape_bits >> 3 & 1;
            sh[SGV_PS_PAIR] = sh[SGV_PS_REST_PAIR] = shape_bits >> 4;
            sh[SGV_PS_WIDE_IDLE] = sh[SGV_PS_NGRP] = sh[SGV_PS_WIDE_NGRP] = sh[SGV_PS_REST_NGRP] = 1;
            int ix[SGV_SW_N] = {};
            for (bool more = true; more;) {
              int32_t sw[SGV_SW_N], form[SGV_PF_N + 1];
              for (int i = 0; i < SGV_SW_N; ++i) sw[i] = sv[i][ix[i]];
              form[SGV_PF_N] = -7;
              bad += sgv_pass_form_model(sh, sw, mm, nc, form, SGV_PF_N + 1) != SGV_OK;
              bad += form[SGV_PF_N] != -7;
              const int k = form[SGV_PF_KIND];
              bad += k < SGV_KIND_VALU || k > SGV_KIND_WALK;
              bad += (k == SGV_KIND_VALU) != (form[SGV_PF_PK_WIDTH] == 0);
              bad += k != SGV_KIND_VALU && nc > form[SGV_PF_PK_WIDTH];
              bad += (k == SGV_KIND_VALU) != (form[SGV_PF_VALU_CLASS] >= 0);
              bad += form[SGV_PF_VALU_CLASS] > 3;
              bad += (k == SGV_KIND_WALK || k == SGV_KIND_WIDE || k == SGV_KIND_PAIR) && nc > 8;
              bad += k == SGV_KIND_WIDE && nc < 3;
              bad += form[SGV_PF_REST_KIND] != SGV_KIND_NONE && k != SGV_KIND_WIDE;
              sgv::PlanShape ps;
              ps.bits = bits;
              ps.packed = true;
              ps.walks = sh[SGV_PS_WALKS];
              ps.wide = sh[SGV_PS_WIDE];
              ps.rest = sh[SGV_PS_REST];
              ps.ragged = ps.rest_ragged = sh[SGV_PS_RAGGED];
              ps.pair = ps.rest_pair = sh[SGV_PS_PAIR];
              sgv::PassSwitches s;
              s.band_walk = sw[0], s.f32_walk = sw[1], s.mf_wide = sw[2], s.mf_pair = sw[3];
              s.mf_wide_idle = sw[4], s.f32_form = sw[5], s.fin_form = sw[6];
              int32_t direct[SGV_PF_N];
              sgv::pass_form_ints(sgv::pass_form(ps, nc, mm, s), direct, SGV_PF_N);
              bad += std::memcmp(direct, form, sizeof direct) != 0;
              ++n_forms;
              more = false;
              for (int i = 0; i < SGV_SW_N && !more; ++i) {
                more = ++ix[i] < sn[i];
                if (!more) ix[i] = 0;
              }
            }
          }
    std::printf("pass forms %ld\n", n_forms);
    bad += n_forms != 2L * 4 * 16 * 48 * 648;
    int32_t sh[SGV_PS_N] = {64}, sw[SGV_SW_N] = {-1, -1, -1, -1, -1, -1, -1}, form[SGV_PF_N];
    bad += sgv_pass_form_model(sh, sw, 3, 0, form, SGV_PF_N) == SGV_OK;
    bad += sgv_pass_form_model(sh, sw, 3, 17, form, SGV_PF_N) == SGV_OK;
    bad += sgv_pass_form_model(nullptr, sw, 3, 4, form, SGV_PF_N) == SGV_OK;
    bad += sgv_pass_form_model(sh, sw, 3, 4, form, 0) != SGV_OK;
    sw[SGV_SW_FIN_FORM] = 2;
    bad += sgv_pass_form_model(sh, sw, 3, 4, form, SGV_PF_N) == SGV_OK;
  }
  std::printf(bad ? "FAILED %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
