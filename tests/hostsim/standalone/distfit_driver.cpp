// distfit_driver — the two entry points of distfit.hip on the host simulation under the compiler's sanitizers (TEST
// INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_distfit_cpu.py links
// it with distfit.hip (thread by thread: a lane's LDS column is private) and sim_runtime.cpp, everything compiled with -g -O1
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// The field is a malloc block of EXACTLY T * C elements, every output one of exactly its rows * C; the LDS block and the work
// buffer are heap blocks of the sizes the entry point asks for.  So a read one row past the field, a staged value past a lane's
// 32 LDS slots or past its work-buffer column, and a level past row nq land in a redzone.  The cases: every distribution and
// method on 1, 65 and 260 cells, float32 and float64, T of 1, 2, 3, 32 and 33, nq of 0 and 16, and nq of 17 (XH_ERR_LIMIT, the
// outputs keep their bytes).  Nelder-Mead on samples of 2 and 3 values has no reference to agree with: what is checked is that
// every parameter is finite or NaN together with its cell, and that the evaluation count respects the budget of 200 N.
#include "driver_common.h"
#include "units/xclim_hip_distfit.h"

const char* const kProgram = "distfit_driver";

namespace {

const uint64_t kPoison = 0x7B7B7B7B7B7B7B7BULL;

bool poison(double v) {
  uint64_t bits;
  memcpy(&bits, &v, 8);
  return bits == kPoison;
}

struct Form {
  int dist, method, has_floc;
  double floc;
};

// every served (distribution, method, floc) form
const Form kForms[] = {
    {XH_DIST_NORM, XH_DIST_ML, 0, 0.0},       {XH_DIST_GUMBEL_R, XH_DIST_ML, 0, 0.0}, {XH_DIST_GENEXTREME, XH_DIST_ML, 0, 0.0},
    {XH_DIST_GENEXTREME, XH_DIST_APP, 0, 0.0}, {XH_DIST_GAMMA, XH_DIST_ML, 0, 0.0},    {XH_DIST_GAMMA, XH_DIST_ML, 1, 0.0},
    {XH_DIST_GAMMA, XH_DIST_ML, 1, -3.0},     {XH_DIST_GAMMA, XH_DIST_APP, 0, 0.0},   {XH_DIST_GAMMA, XH_DIST_APP, 1, 0.0},
    {XH_DIST_FISK, XH_DIST_ML, 0, 0.0},       {XH_DIST_FISK, XH_DIST_ML, 1, -3.0},    {XH_DIST_FISK, XH_DIST_APP, 0, 0.0},
    {XH_DIST_FISK, XH_DIST_APP, 1, -3.0},     {XH_DIST_LOGNORM, XH_DIST_ML, 1, 0.0},  {XH_DIST_LOGNORM, XH_DIST_ML, 1, -3.0},
    {XH_DIST_LOGNORM, XH_DIST_APP, 0, 0.0},   {XH_DIST_LOGNORM, XH_DIST_APP, 1, 0.0},
};

template <typename TE>
void run(const Form& f, int64_t T, int64_t C, int nq) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* x = field<TE>(T, C, 17u + (unsigned)(T * 31 + C + f.dist), 2.0, 40.0);   // EXACTLY (T, C), about one NaN in 97
  if (C > 2)
    for (int64_t t = 0; t < T; ++t) x[t * C + 2] = (TE)NAN;   // a cell with no value
  const int np = (f.dist == XH_DIST_NORM || f.dist == XH_DIST_GUMBEL_R) ? 2 : 3;
  std::vector<double> qs;
  for (int j = 0; j < nq; ++j) qs.push_back((j + 0.5) / (nq > 0 ? nq : 1));
  double* q = exact(qs);
  double* params = block<double>(np * C);
  int32_t* nfev = block<int32_t>(C);
  uint8_t* status = block<uint8_t>(C);
  double* levels = block<double>((int64_t)nq * C);
  const int rc = xh_dist_fit(ctx, x, T, C, C, sizeof(TE) == 8, f.dist, f.method, f.has_floc, f.floc, q, nq, XH_DIST_PPF, params, C, nfev,
                             status, levels, C);
  if (nq > XH_DISTFIT_MAX_Q) {
    if (rc != XH_ERR_LIMIT) fail("one level past the limit is not XH_ERR_LIMIT");
    for (int64_t i = 0; i < np * C; ++i)
      if (!poison(params[i])) fail("a refused call wrote its parameters");
    for (int64_t i = 0; i < (int64_t)nq * C; ++i)
      if (!poison(levels[i])) fail("a refused call wrote its levels");
  } else {
    ok(rc, "xh_dist_fit");
    const int budget = 200 * (f.has_floc ? 2 : 3);
    for (int64_t c = 0; c < C; ++c) {
      int nan = 0;
      for (int k = 0; k < np; ++k) {
        const double v = params[k * C + c];
        if (poison(v)) fail("a parameter was not written");
        nan += v != v;
      }
      if (nan != 0 && nan != np) fail("some, not all, of a cell's parameters are NaN");
      if (status[c] > XH_DISTFIT_SUPPORT) fail("a status byte was not written");
      if ((nan != 0) != (status[c] == XH_DISTFIT_NAN || status[c] == XH_DISTFIT_SUPPORT)) fail("status and NaN parameters disagree");
      if (nfev[c] < 0 || nfev[c] > budget) fail("the evaluation count is outside the budget");
      if ((T <= 1 || (C > 2 && c == 2)) && nan == 0) fail("a cell with fewer than two values is not NaN");
      for (int j = 0; j < nq; ++j) {
        if (poison(levels[(int64_t)j * C + c])) fail("a level was not written");
        if (nan != 0 && levels[(int64_t)j * C + c] == levels[(int64_t)j * C + c]) fail("a level of NaN parameters is not NaN");
      }
    }
    // xh_dist_eval on the parameters: the fused levels bit for bit, and cdf / pdf written everywhere
    if (nq > 0) {
      double* again = block<double>((int64_t)nq * C);
      ok(xh_dist_eval(ctx, f.dist, XH_DIST_PPF, params, C, C, q, nq, again, C), "xh_dist_eval");
      if (memcmp(again, levels, sizeof(double) * (size_t)nq * (size_t)C) != 0) fail("the fused levels differ from xh_dist_eval");
      const std::vector<double> vs = {-1.0, 0.0, 7.5, 60.0};
      double* hv = exact(vs);
      for (int func : {XH_DIST_ISF, XH_DIST_CDF, XH_DIST_PDF}) {
        double* out = block<double>(4 * C);
        ok(xh_dist_eval(ctx, f.dist, func, params, C, C, func == XH_DIST_ISF ? q : hv, 4, out, C), "xh_dist_eval");
        for (int64_t i = 0; i < 4 * C; ++i) {
          if (poison(out[i])) fail("an evaluated element was not written");
          if (func == XH_DIST_CDF && out[i] == out[i] && !(out[i] >= 0.0 && out[i] <= 1.0)) fail("a cdf value lies outside [0, 1]");
        }
        free(out);
      }
      free(hv), free(again);
    }
  }
  free(x), free(q), free(params), free(nfev), free(status), free(levels);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_shapes() {
  for (const Form& f : kForms) {
    for (int64_t C : {1, 65, 260}) run<TE>(f, 33, C, 16);
    for (int64_t T : {1, 2, 3, 32}) run<TE>(f, T, 65, T == 32 ? 16 : 0);   // T = 2, 3: Nelder-Mead on 2 and 3 values
    run<TE>(f, 32, 2, XH_DISTFIT_MAX_Q + 1);
  }
}

}  // namespace

int main() {
  all_shapes<float>();
  all_shapes<double>();
  printf("distfit_driver: %d cases clean\n", g_cases);
  return 0;
}
