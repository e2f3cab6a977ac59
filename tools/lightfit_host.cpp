// robir_amd/csrc/lightfit/lightfit_math.h built for the host: plain loops over pixels and lobes around the same bodies the kernels of
// lightfit.hip loop around, for tools/check_lightfit_host.py (the derivation's check without a GPU).  fp64 outputs, nothing rounded.
#include "lightfit/lightfit_math.h"

#include <vector>

using namespace rb::lf;

namespace {

// the seven sums of every lobe for the upstream r(p, rgb[p]); returns the sum of the squared errors when target is given
template <class Up>
double sums(const float* lgt, int M, const float* dirs, long n, const float* target, double inv_3n, Up up, std::vector<double>& S) {
  std::vector<Lobe> L(M);
  for (int k = 0; k < M; ++k) L[k] = lobe_of(lgt + 7 * k);
  S.assign((size_t)M * 7, 0.0);
  std::vector<double> e(M), cm1(M);
  double sq = 0.0;
  for (long p = 0; p < n; ++p) {
    const double d[3] = {(double)dirs[3 * p], (double)dirs[3 * p + 1], (double)dirs[3 * p + 2]};
    double rgb[3] = {0.0, 0.0, 0.0}, r[3];
    for (int k = 0; k < M; ++k) {
      e[k] = lobe_e(L[k], d, cm1[k]);
      lobe_rgb(L[k], e[k], rgb);
    }
    if (target)
      sq += mse_upstream(rgb, target + 3 * p, inv_3n, r);
    else
      up(p, r);
    for (int k = 0; k < M; ++k) lobe_accum(L[k], d, cm1[k], e[k], r, &S[(size_t)k * 7]);
  }
  return sq;
}

void chain(const float* lgt, int M, const std::vector<double>& S, double* grad) {
  for (int k = 0; k < M; ++k) lobe_chain(lgt + 7 * k, lobe_of(lgt + 7 * k), &S[(size_t)k * 7], grad + 7 * k);
}

}  // namespace

extern "C" {

// d <g_rgb, rgb> / d lgt -> grad [M,7] fp64
void lf_host_bwd(const float* lgt, int M, const float* dirs, long n, const float* g_rgb, double* grad) {
  std::vector<double> S;
  sums(lgt, M, dirs, n, nullptr, 0.0, [&](long p, double* r) { for (int c = 0; c < 3; ++c) r[c] = (double)g_rgb[3 * p + c]; }, S);
  chain(lgt, M, S, grad);
}

// loss = mean((rgb - target)^2) and its gradient [M,7] fp64
double lf_host_loss_grad(const float* lgt, int M, const float* dirs, const float* target, long n, double* grad) {
  std::vector<double> S;
  const double inv_3n = 1.0 / (3.0 * (double)n);
  const double sq = sums(lgt, M, dirs, n, target, inv_3n, [](long, double*) {}, S);
  chain(lgt, M, S, grad);
  return sq * inv_3n;
}

// n_steps fused steps on fp32 parameters and moments, in place; loss_hist[i] = the loss before step i's update
void lf_host_fit(float* lgt, float* adam_m, float* adam_v, int M, const float* dirs, const float* target, long n, long first_step, long n_steps,
                 double lr, double beta1, double beta2, double eps, double* loss_hist) {
  std::vector<double> grad((size_t)M * 7);
  for (long i = 0; i < n_steps; ++i) {
    loss_hist[i] = lf_host_loss_grad(lgt, M, dirs, target, n, grad.data());
    const double t = (double)(first_step + i + 1);
    for (int e = 0; e < 7 * M; ++e)
      adam_element(lgt[e], adam_m[e], adam_v[e], grad[e], lr, beta1, beta2, eps, 1.0 - pow(beta1, t), 1.0 - pow(beta2, t));
  }
}

}  // extern "C"
