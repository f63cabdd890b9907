// qrack_amd — host mathematics of the Krylov calls (LanczosTridiagonal,
// KrylovEvolvePauliSum, LanczosGroundState): everything here is O(dim^3)
// host arithmetic on the projected tridiagonal matrix, shared by every
// engine so that none can drift. No engine, no device and no LAPACK involved.
//
//   Lanczos(dim) on psi, ||psi|| > 0:
//     v_1 = psi / ||psi||, beta_1 = 0
//     for j = 1 .. dim:
//         w          = H v_j - beta_j v_(j-1)
//         alpha_j    = Re <v_j|w>            (Paige's form: after the beta term)
//         w          = w - alpha_j v_j
//         beta_(j+1) = ||w||
//         k = j; stop if j == dim or beta_(j+1) <= theta
//         v_(j+1)    = w / beta_(j+1)
//     theta = 8 (L + 2) eps_R S
//
// S is |identity| plus the summed |weight| of the canonical sum and L its
// launch count. theta is the rounding level of a vanishing w (elementwise
// 4 L eps_R a_j from the apply, one rounding per axpy, a factor 2 of margin):
// a stop there is the happy breakdown, the subspace is invariant. There is no
// re-orthogonalisation.
//
// Engines keep the basis unnormalised: buffer u_j holds the w of step j - 1
// (u_1 is the state) and v_j = s_j u_j with s_j = 1 / beta_j, s_1 = 1 / ||psi||.
// The scale is multiplied into the step's weights here, in double.
#pragma once

#include "common/types.hpp"

#include <cmath>
#include <cstddef>
#include <limits>
#include <utility>
#include <vector>

namespace qrack_amd {

constexpr int KRYLOV_MAX_DIM = 64;
// basis vectors one combine pass adds to the state (the HIP kernel carries
// their pointers in its arguments); a longer basis takes further passes
constexpr int KRYLOV_COMBINE_MAX_VECTORS = 16;

inline double krylovTheta(size_t launches, double epsR, double sumAbs)
{
    return 8.0 * ((double)launches + 2.0) * epsR * sumAbs;
}

// Eigen-decomposition of the real symmetric tridiagonal matrix with diagonal
// alpha (k entries) and off-diagonal beta[0 .. k-2] (further entries of beta
// are ignored, so a Lanczos run's beta_2 .. beta_(k+1) can be passed as it is).
// Cyclic Jacobi on the dense matrix: k <= 64 makes it a few million flops.
// lam is unsorted; vec[i * k + m] is component i of eigenvector m. The
// rotations accumulate one rounding each into the vectors, about 100 per
// column, so the work is done in KrylovReal: with an extended long double
// (x86: 64-bit mantissa) the results are good to the last bit of a double.
// Where long double is a plain double (some ARM and Windows ABIs) everything
// here still works, but exp(-i tau T) e_1 then carries those roundings: about
// 4e-15 at k = 16, which an fp32 state never shows and an fp64 state does.
// The stop test sits far below KrylovReal's own rounding on purpose: Jacobi
// converges quadratically, so the sweep that gets under it is the one after
// the off-diagonal mass reaches rounding level, and 64 sweeps bound the loop.
using KrylovReal = long double;

inline void symTridiagEigen(const std::vector<double>& alpha, const std::vector<double>& beta,
    std::vector<KrylovReal>& lam, std::vector<KrylovReal>& vec)
{
    using T = KrylovReal;
    const size_t k = alpha.size();
    std::vector<T> a(k * k, (T)0);
    vec.assign(k * k, (T)0);
    T total = 0;
    for (size_t i = 0; i < k; ++i) {
        a[i * k + i] = alpha[i];
        vec[i * k + i] = 1;
        total += (T)alpha[i] * alpha[i];
        if (i + 1u < k) {
            a[i * k + i + 1u] = a[(i + 1u) * k + i] = beta[i];
            total += (T)2 * beta[i] * beta[i];
        }
    }
    // off-diagonal mass well below the rounding of the entries themselves
    const T done = std::numeric_limits<T>::epsilon() * std::numeric_limits<T>::epsilon() * (T)1e-4 * total;
    for (int sweep = 0; sweep < 64; ++sweep) {
        T off = 0;
        for (size_t p = 0; p < k; ++p) {
            for (size_t q = p + 1u; q < k; ++q) off += a[p * k + q] * a[p * k + q];
        }
        if (off <= done) break;
        for (size_t p = 0; p < k; ++p) {
            for (size_t q = p + 1u; q < k; ++q) {
                const T apq = a[p * k + q];
                if (apq == 0) continue;
                const T th = (a[q * k + q] - a[p * k + p]) / (2 * apq);
                const T t = (th >= 0 ? (T)1 : (T)-1) / (std::abs(th) + std::sqrt(th * th + 1));
                const T c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (size_t r = 0; r < k; ++r) { // columns p and q
                    const T arp = a[r * k + p], arq = a[r * k + q];
                    a[r * k + p] = c * arp - s * arq;
                    a[r * k + q] = s * arp + c * arq;
                }
                for (size_t r = 0; r < k; ++r) { // rows p and q
                    const T apr = a[p * k + r], aqr = a[q * k + r];
                    a[p * k + r] = c * apr - s * aqr;
                    a[q * k + r] = s * apr + c * aqr;
                }
                a[p * k + q] = a[q * k + p] = 0;
                for (size_t r = 0; r < k; ++r) {
                    const T vrp = vec[r * k + p], vrq = vec[r * k + q];
                    vec[r * k + p] = c * vrp - s * vrq;
                    vec[r * k + q] = s * vrp + c * vrq;
                }
            }
        }
    }
    lam.resize(k);
    for (size_t i = 0; i < k; ++i) lam[i] = a[i * k + i];
}

// c = exp(-i tau T) e_1 for the tridiagonal T of (alpha, beta): unit 2-norm
inline std::vector<cplx<double>> krylovCoefficients(
    const std::vector<double>& alpha, const std::vector<double>& beta, double tau)
{
    const size_t k = alpha.size();
    std::vector<KrylovReal> lam, vec;
    symTridiagEigen(alpha, beta, lam, vec);
    std::vector<KrylovReal> re(k, 0), im(k, 0);
    for (size_t m = 0; m < k; ++m) {
        const KrylovReal cs = std::cos((KrylovReal)tau * lam[m]), sn = -std::sin((KrylovReal)tau * lam[m]);
        const KrylovReal first = vec[m]; // component 0 of eigenvector m
        for (size_t i = 0; i < k; ++i) {
            const KrylovReal f = vec[i * k + m] * first;
            re[i] += f * cs;
            im[i] += f * sn;
        }
    }
    std::vector<cplx<double>> c(k);
    for (size_t i = 0; i < k; ++i) c[i] = cplx<double>((double)re[i], (double)im[i]);
    return c;
}

// lowest eigenpair of the tridiagonal T of (alpha, beta); y has unit 2-norm
inline double krylovLowestRitz(
    const std::vector<double>& alpha, const std::vector<double>& beta, std::vector<double>& y)
{
    const size_t k = alpha.size();
    std::vector<KrylovReal> lam, vec;
    symTridiagEigen(alpha, beta, lam, vec);
    size_t lo = 0;
    for (size_t m = 1; m < k; ++m) {
        if (lam[m] < lam[lo]) lo = m;
    }
    y.resize(k);
    for (size_t i = 0; i < k; ++i) y[i] = (double)vec[i * k + lo];
    return (double)lam[lo];
}

// What a Lanczos run leaves: alpha_1..k, beta_2..(k+1) and the scales s_1..k
// of the unnormalised basis.
struct KrylovRun {
    std::vector<double> alpha, beta, scale;
    double norm0 = 0; // ||psi||
    size_t k() const { return alpha.size(); }
};

// The loop above around an engine's fused step. step(j, s_j, b) forms
//   u_(j+1) = s_j H u_j - b u_(j-1) - a u_j,  a = s_j^2 Re <u_j | s_j H u_j - b u_(j-1)>
// (b = 0 and no u_0 at j = 1; nothing need be stored at j == dim) and returns
// (Re <u_j | s_j H u_j - b u_(j-1)>, ||u_(j+1)||^2).
template <typename StepFn>
inline KrylovRun lanczosDrive(int dim, double norm0, double theta, StepFn&& step)
{
    KrylovRun run;
    run.norm0 = norm0;
    double s = 1.0 / norm0, sPrev = 0, beta = 0;
    for (int j = 1; j <= dim; ++j) {
        const std::pair<double, double> r = step(j, s, beta * sPrev);
        run.alpha.push_back(s * r.first);
        run.scale.push_back(s);
        beta = std::sqrt(r.second > 0 ? r.second : 0.0);
        run.beta.push_back(beta);
        if (j == dim || !(beta > theta)) break;
        sPrev = s;
        s = 1.0 / beta;
    }
    return run;
}

} // namespace qrack_amd
