// qrack_amd — host mathematics of the Krylov calls (LanczosTridiagonal,
// KrylovEvolvePauliSum, LanczosGroundState, LanczosLowestStates): everything
// here is O(dim^3) host arithmetic on the projected matrix, shared by every
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
//
// LanczosLowestStates is a thick-restart Lanczos with full re-orthogonalisation
// (Wu and Simon, SIAM J. Matrix Anal. Appl. 22, 2000), for the nev lowest
// eigenpairs. 1 <= nev <= KRYLOV_EIG_MAX_NEV, nev + 2 <= dim <= KRYLOV_MAX_DIM,
// tol >= 0 (absolute, units of H), maxRestarts >= 0, -1 <= prepare < nev.
//
//   threshold = max(tol, theta)          (theta as above)
//   keep      = min(2 nev, nev + (dim - nev) / 2, dim - 2)     (integer division)
//
//   Orth(w, V = [v_1..v_j]):  for round r = 1, 2
//                               for chunks g of CAP = 16 consecutive vectors, in order
//                                   c_g = V_g^H w;  w <- w - V_g c_g
//                             h_i = the sum of c_i over both rounds (complex)
//
//   cycle 0: v_1 = psi / ||psi||, j = 1
//   step j:  w = H v_j                   (no beta term: Orth removes it)
//            (w, h) = Orth(w, [v_1..v_j])
//            T[j,j] = Re h_j, beta_(j+1) = ||w||, k = j
//            the cycle stops at k == dim or at breakdown, beta_(k+1) <= theta;
//            else T[j,j+1] = T[j+1,j] = beta_(j+1), v_(j+1) = w / beta_(j+1)
//   end of a cycle:
//            T[:k,:k] = S diag(lambda) S^T, lambda ascending (Jacobi, KrylovReal)
//            res_i = beta_(k+1) |S[k-1,i]|;  the lowest m = min(nev, k) pairs
//            join the history. The call ends on breakdown, when all m residuals
//            are <= threshold, or when the cycle number equals maxRestarts;
//            converged = (m == nev and all residuals <= threshold).
//   restart: kp = min(keep, k);  v~_i = V S[:,i] for i < kp;  v~_(kp+1) = w / beta_(k+1)
//            T~ = diag(lambda_0..lambda_(kp-1)), T~[i,kp] = T~[kp,i] = beta_(k+1) S[k-1,i]
//            (host values, not measured inner products); go on with step kp + 1.
//   prepare = i leaves V S[:,i] of the final cycle in the simulator (unit norm
//   by the basis's orthonormality); prepare = -1 leaves the state bit-identical.
//   A pair the run did not produce (i >= m) is refused, the state intact.
//
// A single start vector finds each eigenspace once: a degenerate level appears
// once, and a start vector inside a symmetry sector finds that sector's levels.
//
// Here too the engines keep the basis unnormalised, v_i = s_i u_i: Orth's
// coefficient of u_i is s_i^2 <u_i|w>, h_i = s_i <u_i|w>, and the restart
// folds the s_i into the rotation, whose outputs have s = 1.
#pragma once

#include "common/types.hpp"

#include <algorithm>
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

// The cyclic Jacobi sweeps on the dense symmetric k x k matrix `a` (row-major,
// overwritten); `total` is the squared Frobenius mass the stop test scales by.
inline void symJacobiSweeps(std::vector<KrylovReal>& a, size_t k, KrylovReal total, std::vector<KrylovReal>& lam,
    std::vector<KrylovReal>& vec)
{
    using T = KrylovReal;
    vec.assign(k * k, (T)0);
    for (size_t i = 0; i < k; ++i) vec[i * k + i] = 1;
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

// the tridiagonal of (alpha, beta), as described above
inline void symTridiagEigen(const std::vector<double>& alpha, const std::vector<double>& beta,
    std::vector<KrylovReal>& lam, std::vector<KrylovReal>& vec)
{
    using T = KrylovReal;
    const size_t k = alpha.size();
    std::vector<T> a(k * k, (T)0);
    T total = 0;
    for (size_t i = 0; i < k; ++i) {
        a[i * k + i] = alpha[i];
        total += (T)alpha[i] * alpha[i];
        if (i + 1u < k) {
            a[i * k + i + 1u] = a[(i + 1u) * k + i] = beta[i];
            total += (T)2 * beta[i] * beta[i];
        }
    }
    symJacobiSweeps(a, k, total, lam, vec);
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

// ---- LanczosLowestStates ---------------------------------------------------------

constexpr int KRYLOV_EIG_MAX_NEV = 8;
// vectors one orthogonalisation launch handles: the CAP of the definition
constexpr int KRYLOV_ORTH_MAX_VECTORS = 16;
static_assert(2 * KRYLOV_EIG_MAX_NEV <= KRYLOV_COMBINE_MAX_VECTORS, "keep <= 2 nev fits one rotation");

struct KrylovEigenResult {
    std::vector<double> values;    // ascending, min(nev, k) entries
    std::vector<double> residuals; // beta_(k+1) |S[k-1, i]| of the same pairs
    bool converged = false;        // nev pairs returned, all residuals <= threshold
    int restarts = 0;              // cycles run after cycle 0
    int applies = 0;               // applications of H
    // (restarts + 1) rows of nev, NaN-padded
    std::vector<double> historyValues, historyResiduals;
};

inline int krylovEigenKeep(int nev, int dim)
{
    return std::min(std::min(2 * nev, nev + (dim - nev) / 2), dim - 2);
}

// launches of Orth against j vectors. One chunk: inner products, update fused
// with the second round's inner products, update fused with the norm. More
// chunks: the defined order has no such pairs (a chunk's inner products follow
// the update of another chunk), so every (round, chunk) is an inner-product
// launch and an update launch; the last update also leaves the norm.
inline int krylovOrthLaunches(int j)
{
    const int chunks = (j + KRYLOV_ORTH_MAX_VECTORS - 1) / KRYLOV_ORTH_MAX_VECTORS;
    return chunks == 1 ? 3 : 4 * chunks;
}

// what a step hands back: h_1..h_j (both rounds summed, in units of the
// normalised basis) and ||w||^2
struct KrylovOrthStep {
    std::vector<cplx<double>> h;
    double norm2 = 0;
};

struct KrylovEigenRun {
    KrylovEigenResult result;
    // prepare >= 0: coefficients of u_1..u_k of the final cycle's basis (the
    // scales folded in); empty when the run has no such pair
    std::vector<double> prepareCoef;
    // basis vectors the engine holds at the end: k of the final cycle
    int k = 0;
};

// The definition above around three engine callbacks.
//   step(j, scale)     w = s_j H u_j, Orth against u_1..u_j whose scales are
//                      scale[0..j-1]; returns KrylovOrthStep
//   accept()           the w of the last step becomes u_(j+1)
//   rotate(k, kp, m)   u~_i = sum_r m[r * kp + i] u_r for i < kp, then the w of
//                      the last step becomes u~_(kp+1); the outputs replace the basis
template <typename StepFn, typename AcceptFn, typename RotateFn>
inline KrylovEigenRun krylovEigenDrive(int nev, int dim, double tol, int maxRestarts, int prepare, double norm0,
    double theta, StepFn&& step, AcceptFn&& accept, RotateFn&& rotate)
{
    KrylovEigenRun run;
    KrylovEigenResult& out = run.result;
    const double threshold = std::max(tol, theta);
    const int keep = krylovEigenKeep(nev, dim);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t d = (size_t)dim;
    std::vector<double> t(d * d, 0.0), scale(1, 1.0 / norm0);
    int j = 1;
    for (int cycle = 0;; ++cycle) {
        bool broke = false;
        double beta = 0;
        int k = 0;
        for (;;) {
            const KrylovOrthStep r = step(j, scale);
            ++out.applies;
            t[(size_t)(j - 1) * d + (size_t)(j - 1)] = r.h[(size_t)(j - 1)].re;
            beta = std::sqrt(r.norm2 > 0 ? r.norm2 : 0.0);
            k = j;
            if (!(beta > theta)) {
                broke = true;
                break;
            }
            if (k == dim) break;
            t[(size_t)(j - 1) * d + (size_t)j] = t[(size_t)j * d + (size_t)(j - 1)] = beta;
            accept();
            scale.push_back(1.0 / beta);
            ++j;
        }
        const size_t kk = (size_t)k;
        std::vector<KrylovReal> a(kk * kk), lam, vec;
        KrylovReal total = 0;
        for (size_t p = 0; p < kk; ++p) {
            for (size_t q = 0; q < kk; ++q) {
                a[p * kk + q] = t[p * d + q];
                total += a[p * kk + q] * a[p * kk + q];
            }
        }
        symJacobiSweeps(a, kk, total, lam, vec);
        std::vector<size_t> order(kk);
        for (size_t i = 0; i < kk; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lam[x] < lam[y]; });
        const int m = std::min(nev, k);
        bool allUnder = true;
        std::vector<double> values((size_t)m), residuals((size_t)m);
        for (int i = 0; i < m; ++i) {
            values[(size_t)i] = (double)lam[order[(size_t)i]];
            residuals[(size_t)i] = beta * (double)std::abs(vec[(kk - 1u) * kk + order[(size_t)i]]);
            if (!(residuals[(size_t)i] <= threshold)) allUnder = false;
        }
        for (int i = 0; i < nev; ++i) {
            out.historyValues.push_back(i < m ? values[(size_t)i] : nan);
            out.historyResiduals.push_back(i < m ? residuals[(size_t)i] : nan);
        }
        if (broke || allUnder || cycle == maxRestarts) {
            out.values = values;
            out.residuals = residuals;
            out.converged = (m == nev) && allUnder;
            out.restarts = cycle;
            run.k = k;
            if (prepare >= 0 && prepare < m) {
                run.prepareCoef.resize(kk);
                for (size_t r = 0; r < kk; ++r) {
                    run.prepareCoef[r] = (double)(vec[r * kk + order[(size_t)prepare]] * (KrylovReal)scale[r]);
                }
            }
            return run;
        }
        const int kp = std::min(keep, k);
        std::vector<double> rot(kk * (size_t)kp);
        for (size_t r = 0; r < kk; ++r) {
            for (int i = 0; i < kp; ++i) {
                rot[r * (size_t)kp + (size_t)i] = (double)(vec[r * kk + order[(size_t)i]] * (KrylovReal)scale[r]);
            }
        }
        rotate(k, kp, rot);
        std::fill(t.begin(), t.end(), 0.0);
        for (int i = 0; i < kp; ++i) {
            t[(size_t)i * d + (size_t)i] = (double)lam[order[(size_t)i]];
            t[(size_t)i * d + (size_t)kp] = t[(size_t)kp * d + (size_t)i]
                = beta * (double)vec[(kk - 1u) * kk + order[(size_t)i]];
        }
        scale.assign((size_t)kp, 1.0);
        scale.push_back(1.0 / beta);
        j = kp + 1;
    }
}

} // namespace qrack_amd
