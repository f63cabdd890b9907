// qrack_amd — CDNA4 (gfx950) device kernels for the HIP state-vector engine.
//
// Parity target: the reference kernel inventory in
// /root/reference/src/common/qengine.cl + qheader_alu.cl,
// re-designed for MI355X rather than translated:
//  - wave64 blocks (256 threads), grid-stride loops capped at ~8 blocks/CU;
//  - fp32 amplitude streams vectorized as float4 (two complex amps per lane,
//    16 B/lane — G13 of the CDNA HIP guide); fp64 is naturally 16 B/lane;
//  - reductions: wave shuffle (64-wide) -> LDS across the block's 4 waves ->
//    one partial per block, finished on host (no global atomics);
//  - the entire ALU family is ONE uniform-opcode permutation kernel (the
//    branch is wave-uniform) instead of 26 near-identical kernels.
#include "kernels.hpp"
#include "qft_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

namespace qrack_amd {

#ifndef QA_BLOCK_OVERRIDE
constexpr int QA_BLOCK = 256;
#else
constexpr int QA_BLOCK = QA_BLOCK_OVERRIDE;
#endif
// Streaming gate kernels launch an EXACT grid (one iteration per thread):
// the block-count A/B on the 30q QFT is monotone all the way up —
// 2048 = 112.1 ms, 8192 = 108.0, 32768 = 104.4, exact (~0.5-1M blocks) =
// 96.0 ms. Consecutive blocks touch consecutive tiles, which keeps each
// XCD's L2 on a contiguous slice; the grid-stride remainder loop only
// handles env-capped experiments (QRACK_GPU_BLOCKS). Reductions stay
// capped at QA_REDUCE_MAX_BLOCKS to bound their partials buffers.
constexpr int QA_MAX_BLOCKS = QA_REDUCE_MAX_BLOCKS;
// the HSA dispatch packet's grid size is a 32-bit WORK-ITEM count: blocks
// * QA_BLOCK must stay below 2^32 or the launch silently wraps (caught at
// 34 qubits, where the exact column grid needs exactly 2^32 threads)
constexpr bitCapInt QA_GRID_HW_MAX = ((bitCapInt)1 << 24) - 1u;

static inline int maxBlocks()
{
    static int v = [] {
        if (const char* env = std::getenv("QRACK_GPU_BLOCKS")) return std::atoi(env);
        return 0; // 0 = exact grid
    }();
    return v;
}

static inline bool useNontemporal()
{
    static bool v = [] {
        if (const char* env = std::getenv("QRACK_GPU_NT")) return std::atoi(env) != 0;
        return false;
    }();
    return v;
}

static inline int gridFor(bitCapInt n)
{
    bitCapInt b = (n + QA_BLOCK - 1) / QA_BLOCK;
    const int cap = maxBlocks();
    if (cap > 0 && b > (bitCapInt)cap) b = cap;
    if (b > QA_GRID_HW_MAX) b = QA_GRID_HW_MAX;
    if (b < 1) b = 1;
    return (int)b;
}

// one block per LDS tile, up to QA_MAX_BLOCKS and the QRACK_GPU_BLOCKS cap:
// the LDS gate-batch and QFT kernels loop over the remaining tiles
static inline int ldsGridFor(bitCapInt nTiles)
{
    bitCapInt b = std::min<bitCapInt>(nTiles, (bitCapInt)QA_MAX_BLOCKS);
    const int cap = maxBlocks();
    if (cap > 0 && b > (bitCapInt)cap) b = cap;
    return (int)b;
}

// nontemporal (streaming) load/store option for the pure-stream kernels:
// state-vector gate traffic has zero reuse, so bypassing L2/LLC can help
typedef float nat_float4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ float4 ld4(const float4* p)
{
    if constexpr (NT) {
        const nat_float4 v = __builtin_nontemporal_load(reinterpret_cast<const nat_float4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    return *p;
}
template <bool NT> __device__ __forceinline__ void st4(float4* p, float4 v)
{
    if constexpr (NT) {
        nat_float4 nv = { v.x, v.y, v.z, v.w };
        __builtin_nontemporal_store(nv, reinterpret_cast<nat_float4*>(p));
    } else {
        *p = v;
    }
}

// reductions/argmax/inner write one partial PER BLOCK: their grids must
// stay within the fixed partials buffers regardless of the exact-grid
// default for streaming kernels
static inline int gridForReduce(bitCapInt n)
{
    bitCapInt b = (n + QA_BLOCK - 1) / QA_BLOCK;
    if (b > (bitCapInt)QA_REDUCE_MAX_BLOCKS) b = QA_REDUCE_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

int reduceGridSize(bitCapInt n) { return gridForReduce(n); }

__device__ __forceinline__ bitCapInt expandBits(bitCapInt j, const bitCapInt* pows, int n)
{
    for (int k = 0; k < n; ++k) {
        j = ((j & ~(pows[k] - 1u)) << 1u) | (j & (pows[k] - 1u));
    }
    return j;
}

// ---- gate apply -------------------------------------------------------------

// KIND: 0 = generic 2x2, 1 = phase (diagonal), 2 = invert (antidiagonal)
template <typename R, int KIND> __global__ void k_apply2x2(cplx<R>* sv, GateArgs<R> a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < a.maxI; j += stride) {
        const bitCapInt i = expandBits(j, a.qPowers, a.nPowers);
        const bitCapInt i1 = i | a.offset1;
        const bitCapInt i2 = i | a.offset2;
        if (KIND == 1) {
            sv[i1] = a.m[0] * sv[i1];
            sv[i2] = a.m[3] * sv[i2];
        } else if (KIND == 2) {
            const cplx<R> t = sv[i1];
            sv[i1] = a.m[1] * sv[i2];
            sv[i2] = a.m[2] * t;
        } else {
            const cplx<R> x = sv[i1];
            const cplx<R> y = sv[i2];
            sv[i1] = a.m[0] * x + a.m[1] * y;
            sv[i2] = a.m[2] * x + a.m[3] * y;
        }
    }
}

// fp32 vectorized single-target path: each lane handles TWO adjacent pairs
// through float4 (16 B) loads/stores. Requires nPowers == 1 and even maxI.
template <int KIND, bool NT> __global__ void k_apply2x2_1v(cplx<float>* sv, GateArgs<float> a)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt p = a.qPowers[0];
    const bitCapInt half = a.maxI >> 1u; // float4-pair iterations
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const cplx<float> m0 = a.m[0], m1 = a.m[1], m2 = a.m[2], m3 = a.m[3];
    if (p == 1u) {
        // target bit 0: each pair is adjacent = one float4
        for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
            // two pairs: float4s at 2k and 2k+1
            for (int h = 0; h < 2; ++h) {
                const bitCapInt idx = 2u * k + h;
                float4 v = ld4<NT>(&sv4[idx]);
                const cplx<float> x{ v.x, v.y }, y{ v.z, v.w };
                cplx<float> nx, ny;
                if (KIND == 1) {
                    nx = m0 * x;
                    ny = m3 * y;
                } else if (KIND == 2) {
                    nx = m1 * y;
                    ny = m2 * x;
                } else {
                    nx = m0 * x + m1 * y;
                    ny = m2 * x + m3 * y;
                }
                st4<NT>(&sv4[idx], make_float4(nx.re, nx.im, ny.re, ny.im));
            }
        }
    } else {
        // target bit >= 1: pairs (i, i+p); two consecutive j share the block
        for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
            const bitCapInt j = 2u * k;
            const bitCapInt i = ((j & ~(p - 1u)) << 1u) | (j & (p - 1u));
            const bitCapInt lo4 = i >> 1u;       // float4 index of (i, i+1)
            const bitCapInt hi4 = (i + p) >> 1u; // float4 index of (i+p, i+p+1)
            float4 vlo = ld4<NT>(&sv4[lo4]);
            float4 vhi = ld4<NT>(&sv4[hi4]);
            const cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
            const cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
            cplx<float> a0, a1, b0, b1;
            if (KIND == 1) {
                a0 = m0 * x0; a1 = m0 * x1;
                b0 = m3 * y0; b1 = m3 * y1;
            } else if (KIND == 2) {
                a0 = m1 * y0; a1 = m1 * y1;
                b0 = m2 * x0; b1 = m2 * x1;
            } else {
                a0 = m0 * x0 + m1 * y0; a1 = m0 * x1 + m1 * y1;
                b0 = m2 * x0 + m3 * y0; b1 = m2 * x1 + m3 * y1;
            }
            st4<NT>(&sv4[lo4], make_float4(a0.re, a0.im, a1.re, a1.im));
            st4<NT>(&sv4[hi4], make_float4(b0.re, b0.im, b1.re, b1.im));
        }
    }
}

// wide fp32 single-target variant: FOUR adjacent pairs (two float4 per side,
// 32 B/lane/side) — A/B candidate for the HBM-bound H stream
template <int KIND> __global__ void k_apply2x2_1w(cplx<float>* sv, GateArgs<float> a)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt p = a.qPowers[0];
    const bitCapInt quarter = a.maxI >> 2u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const cplx<float> m0 = a.m[0], m1 = a.m[1], m2 = a.m[2], m3 = a.m[3];
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < quarter; k += stride) {
        const bitCapInt j = 4u * k;
        const bitCapInt i = ((j & ~(p - 1u)) << 1u) | (j & (p - 1u));
        const bitCapInt lo4 = i >> 1u;
        const bitCapInt hi4 = (i + p) >> 1u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 vlo = sv4[lo4 + h];
            float4 vhi = sv4[hi4 + h];
            const cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
            const cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
            cplx<float> a0, a1, b0, b1;
            if (KIND == 1) {
                a0 = m0 * x0; a1 = m0 * x1;
                b0 = m3 * y0; b1 = m3 * y1;
            } else if (KIND == 2) {
                a0 = m1 * y0; a1 = m1 * y1;
                b0 = m2 * x0; b1 = m2 * x1;
            } else {
                a0 = m0 * x0 + m1 * y0; a1 = m0 * x1 + m1 * y1;
                b0 = m2 * x0 + m3 * y0; b1 = m2 * x1 + m3 * y1;
            }
            sv4[lo4 + h] = make_float4(a0.re, a0.im, a1.re, a1.im);
            sv4[hi4 + h] = make_float4(b0.re, b0.im, b1.re, b1.im);
        }
    }
}

static inline int wideMode()
{
    static int v = [] {
        if (const char* env = std::getenv("QRACK_GPU_WIDE")) return std::atoi(env);
        return 0;
    }();
    return v;
}

// one-sided diagonal scale: sv[i|offset] *= f for every expanded i.
// The dominant QFT kernel: CPhase(topLeft=1) touches only the
// control=1 & target=1 quarter of the state (the reference's phasesingle
// touches half; this is the MI355X-native improvement).
template <typename R> __global__ void k_scale_side(cplx<R>* sv, GateArgs<R> a, cplx<R> f)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < a.maxI; j += stride) {
        const bitCapInt i = expandBits(j, a.qPowers, a.nPowers) | a.offset1;
        sv[i] = f * sv[i];
    }
}

// fp32 vectorized one-sided scale: two adjacent expanded indices per lane
// (requires qPowers[0] >= 2 so consecutive j stay adjacent, and even maxI)
__global__ void k_scale_side_v(cplx<float>* sv, GateArgs<float> a, cplx<float> f)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt half = a.maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
        const bitCapInt i = (expandBits(2u * k, a.qPowers, a.nPowers) | a.offset1) >> 1u;
        float4 v = sv4[i];
        const cplx<float> x{ v.x, v.y }, y{ v.z, v.w };
        const cplx<float> nx = f * x, ny = f * y;
        sv4[i] = make_float4(nx.re, nx.im, ny.re, ny.im);
    }
}

// fp32 vectorized general/phase/invert pair kernel for ANY skip set with
// qPowers[0] >= 2: two adjacent pairs per lane via float4
template <int KIND> __global__ void k_apply2x2_v(cplx<float>* sv, GateArgs<float> a)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt half = a.maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const cplx<float> m0 = a.m[0], m1 = a.m[1], m2 = a.m[2], m3 = a.m[3];
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
        const bitCapInt i = expandBits(2u * k, a.qPowers, a.nPowers);
        const bitCapInt lo4 = (i | a.offset1) >> 1u;
        const bitCapInt hi4 = (i | a.offset2) >> 1u;
        float4 vlo = sv4[lo4];
        float4 vhi = sv4[hi4];
        const cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
        const cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
        cplx<float> a0, a1, b0, b1;
        if (KIND == 1) {
            a0 = m0 * x0; a1 = m0 * x1;
            b0 = m3 * y0; b1 = m3 * y1;
        } else if (KIND == 2) {
            a0 = m1 * y0; a1 = m1 * y1;
            b0 = m2 * x0; b1 = m2 * x1;
        } else {
            a0 = m0 * x0 + m1 * y0; a1 = m0 * x1 + m1 * y1;
            b0 = m2 * x0 + m3 * y0; b1 = m2 * x1 + m3 * y1;
        }
        sv4[lo4] = make_float4(a0.re, a0.im, a1.re, a1.im);
        sv4[hi4] = make_float4(b0.re, b0.im, b1.re, b1.im);
    }
}

template <typename R> static bool isOne(cplx<R> c) { return c.re == (R)1 && c.im == (R)0; }

template <typename R> static int matrixKind(const cplx<R>* m)
{
    const bool isPhase = (norm(m[1]) <= 0) && (norm(m[2]) <= 0);
    const bool isInvert = (norm(m[0]) <= 0) && (norm(m[3]) <= 0);
    return isPhase ? 1 : (isInvert ? 2 : 0);
}

__global__ void k_apply2x2_1mfma(cplx<float>* sv, GateArgs<float> a);

template <typename R>
void launchApply2x2(cplx<R>* sv, const GateArgs<R>& a, hipStream_t stream)
{
    const int kind = matrixKind(a.m);
    const int grid = gridFor(a.maxI);
    if constexpr (std::is_same_v<R, float>) {
        static const bool useMfma = []() {
            if (const char* env = std::getenv("QRACK_GPU_MFMA")) return std::atoi(env) != 0;
            return false;
        }();
        if (useMfma && a.nPowers == 1) {
            hipLaunchKernelGGL((k_apply2x2_1mfma), dim3(gridFor(a.maxI >> 2u)), dim3(QA_BLOCK), 0,
                stream, sv, a);
            return;
        }
    }
    // fp32 pairs can vectorize as float4 whenever consecutive iteration
    // indices stay memory-adjacent: lowest skip power >= 2
    const bool vecOk = (a.nPowers > 0) && (a.qPowers[0] >= 2u) && ((a.maxI & 1u) == 0u);

    if (kind == 1) {
        // diagonal: skip untouched sides entirely
        const bool tl1 = isOne(a.m[0]);
        const bool br1 = isOne(a.m[3]);
        if (tl1 && br1) return; // identity
        if (tl1 || br1) {
            GateArgs<R> s = a;
            s.offset1 = tl1 ? a.offset2 : a.offset1;
            const cplx<R> f = tl1 ? a.m[3] : a.m[0];
            if constexpr (std::is_same_v<R, float>) {
                if (vecOk) {
                    hipLaunchKernelGGL((k_scale_side_v), dim3(gridFor(a.maxI >> 1u)),
                        dim3(QA_BLOCK), 0, stream, sv, s, f);
                    return;
                }
            }
            hipLaunchKernelGGL(
                (k_scale_side<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, s, f);
            return;
        }
    }
    if constexpr (std::is_same_v<R, float>) {
        if (a.nPowers == 1 && (a.maxI & 1u) == 0u && a.maxI >= 2u && a.offset1 == 0u) {
            // single-target fast path (handles target bit 0 too)
            if (wideMode() && a.qPowers[0] >= 4u && (a.maxI & 3u) == 0u) {
                const int gridw = gridFor(a.maxI >> 2u);
                switch (kind) {
                case 1:
                    hipLaunchKernelGGL((k_apply2x2_1w<1>), dim3(gridw), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                case 2:
                    hipLaunchKernelGGL((k_apply2x2_1w<2>), dim3(gridw), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                default:
                    hipLaunchKernelGGL((k_apply2x2_1w<0>), dim3(gridw), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                }
            }
            const int gridv = gridFor(a.maxI >> 1u);
            if (useNontemporal()) {
                switch (kind) {
                case 1:
                    hipLaunchKernelGGL((k_apply2x2_1v<1, true>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                case 2:
                    hipLaunchKernelGGL((k_apply2x2_1v<2, true>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                default:
                    hipLaunchKernelGGL((k_apply2x2_1v<0, true>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                    return;
                }
            }
            switch (kind) {
            case 1:
                hipLaunchKernelGGL((k_apply2x2_1v<1, false>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            case 2:
                hipLaunchKernelGGL((k_apply2x2_1v<2, false>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            default:
                hipLaunchKernelGGL((k_apply2x2_1v<0, false>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            }
        }
        if (vecOk) {
            const int gridv = gridFor(a.maxI >> 1u);
            switch (kind) {
            case 1:
                hipLaunchKernelGGL((k_apply2x2_v<1>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            case 2:
                hipLaunchKernelGGL((k_apply2x2_v<2>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            default:
                hipLaunchKernelGGL((k_apply2x2_v<0>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            }
        }
    }
    switch (kind) {
    case 1:
        hipLaunchKernelGGL((k_apply2x2<R, 1>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    case 2:
        hipLaunchKernelGGL((k_apply2x2<R, 2>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    default:
        hipLaunchKernelGGL((k_apply2x2<R, 0>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    }
}

// ---- multiplexer ------------------------------------------------------------

template <typename R>
__global__ void k_uniformly_ctrl(cplx<R>* sv, bitCapInt maxI, bitCapInt targetPower,
    const bitCapInt* ctrlPowers, int nCtrls, const cplx<R>* mtrxs)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < maxI; j += stride) {
        const bitCapInt i = ((j & ~(targetPower - 1u)) << 1u) | (j & (targetPower - 1u));
        bitCapInt sel = 0;
        for (int b = 0; b < nCtrls; ++b) {
            if (i & ctrlPowers[b]) sel |= (ONE_BCI << b);
        }
        const cplx<R>* m = mtrxs + 4u * sel;
        const cplx<R> x = sv[i];
        const cplx<R> y = sv[i | targetPower];
        sv[i] = m[0] * x + m[1] * y;
        sv[i | targetPower] = m[2] * x + m[3] * y;
    }
}

template <typename R>
void launchUniformlyControlled(cplx<R>* sv, bitCapInt maxI, bitCapInt targetPower,
    const bitCapInt* ctrlPowersDev, int nCtrls, const cplx<R>* mtrxsDev, hipStream_t stream)
{
    hipLaunchKernelGGL((k_uniformly_ctrl<R>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0, stream, sv,
        maxI, targetPower, ctrlPowersDev, nCtrls, mtrxsDev);
}

// ---- mask gates -------------------------------------------------------------

template <typename R> __global__ void k_xmask(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        const bitCapInt j = i ^ mask;
        if (i < j) {
            const cplx<R> t = sv[i];
            sv[i] = sv[j];
            sv[j] = t;
        }
    }
}

template <typename R>
void launchXMask(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, hipStream_t stream)
{
    hipLaunchKernelGGL(
        (k_xmask<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv, maxQPower, mask);
}

template <typename R>
__global__ void k_parityphase(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, cplx<R> even, cplx<R> odd)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        sv[i] = (__popcll(i & mask) & 1 ? odd : even) * sv[i];
    }
}

template <typename R>
void launchParityPhase(
    cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, cplx<R> even, cplx<R> odd, hipStream_t stream)
{
    hipLaunchKernelGGL((k_parityphase<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv,
        maxQPower, mask, even, odd);
}

// ---- reductions --------------------------------------------------------------

__device__ __forceinline__ double waveReduceSum(double v)
{
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}

template <typename R> __global__ void k_reduce(const cplx<R>* sv, ReduceArgs a, int op, double* partials)
{
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < a.maxI; i += stride) {
        const double n = (double)norm(sv[i]);
        switch ((ReduceOp)op) {
        case ReduceOp::NORM_ALL:
            s += n;
            break;
        case ReduceOp::PROB_BITSET:
            if ((i & a.mask) == a.mask) s += n;
            break;
        case ReduceOp::PROB_MASK:
            if ((i & a.mask) == a.perm) s += n;
            break;
        case ReduceOp::PROB_PARITY:
            if (__popcll(i & a.mask) & 1) s += n;
            break;
        case ReduceOp::EXP_PERM:
        case ReduceOp::EXP_PERM_SQ: {
            double val = a.offset;
            for (int b = 0; b < a.nBits; ++b) {
                if ((i >> a.bitsArr[b]) & 1u) val += (double)a.permsArr[b];
            }
            s += ((ReduceOp)op == ReduceOp::EXP_PERM) ? val * n : val * val * n;
            break;
        }
        case ReduceOp::NORM_FLOOR:
            if (n >= a.normThresh) s += n;
            break;
        }
    }
    s = waveReduceSum(s);
    __shared__ double waveSums[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) waveSums[wid] = s;
    __syncthreads();
    if (wid == 0) {
        double t = (lane < QA_BLOCK / 64) ? waveSums[lane] : 0.0;
        t = waveReduceSum(t);
        if (lane == 0) partials[blockIdx.x] = t;
    }
}

template <typename R>
int launchReduce(const cplx<R>* sv, const ReduceArgs& a, int op, double* partialsDev,
    hipStream_t stream)
{
    const int grid = gridForReduce(a.maxI);
    hipLaunchKernelGGL(
        (k_reduce<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a, op, partialsDev);
    return grid;
}

template <typename R>
__global__ void k_argmax(const cplx<R>* sv, bitCapInt maxI, double* vals, bitCapInt* idxs)
{
    double best = -1.0;
    bitCapInt bestI = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxI; i += stride) {
        const double n = (double)norm(sv[i]);
        if (n > best) {
            best = n;
            bestI = i;
        }
    }
    for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_down(best, off);
        const bitCapInt oi = (bitCapInt)__shfl_down((unsigned long long)bestI, off);
        if (ov > best) {
            best = ov;
            bestI = oi;
        }
    }
    __shared__ double wv[QA_BLOCK / 64];
    __shared__ bitCapInt wi[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) {
        wv[wid] = best;
        wi[wid] = bestI;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < QA_BLOCK / 64; ++k) {
            if (wv[k] > wv[0]) {
                wv[0] = wv[k];
                wi[0] = wi[k];
            }
        }
        vals[blockIdx.x] = wv[0];
        idxs[blockIdx.x] = wi[0];
    }
}

template <typename R>
int launchArgMax(const cplx<R>* sv, bitCapInt maxI, double* valsDev, bitCapInt* idxDev,
    hipStream_t stream)
{
    const int grid = gridForReduce(maxI);
    hipLaunchKernelGGL(
        (k_argmax<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, maxI, valsDev, idxDev);
    return grid;
}

// ---- normalize / projection --------------------------------------------------

template <typename R>
__global__ void k_normalize(cplx<R>* sv, bitCapInt maxQPower, cplx<R> factor, R normThresh)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        const cplx<R> v = sv[i];
        sv[i] = (norm(v) < normThresh) ? cplx<R>(0, 0) : factor * v;
    }
}

template <typename R>
void launchNormalize(cplx<R>* sv, bitCapInt maxQPower, cplx<R> factor, R normThresh, hipStream_t stream)
{
    hipLaunchKernelGGL((k_normalize<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv,
        maxQPower, factor, normThresh);
}

template <typename R>
__global__ void k_applym(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, bitCapInt result, cplx<R> nrm)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        sv[i] = ((i & mask) == result) ? nrm * sv[i] : cplx<R>(0, 0);
    }
}

template <typename R>
void launchApplyM(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, bitCapInt result, cplx<R> nrm,
    hipStream_t stream)
{
    hipLaunchKernelGGL((k_applym<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv,
        maxQPower, mask, result, nrm);
}

template <typename R>
__global__ void k_applyparity(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, int odd, cplx<R> nrm)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        sv[i] = ((__popcll(i & mask) & 1) == odd) ? nrm * sv[i] : cplx<R>(0, 0);
    }
}

template <typename R>
void launchApplyParity(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, bool odd, cplx<R> nrm,
    hipStream_t stream)
{
    hipLaunchKernelGGL((k_applyparity<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv,
        maxQPower, mask, odd ? 1 : 0, nrm);
}

// ---- structural ---------------------------------------------------------------

template <typename R>
__global__ void k_compose(const cplx<R>* a, const cplx<R>* b, cplx<R>* out, bitCapInt nMaxQPower,
    bitLenInt start, bitLenInt oQubits)
{
    const bitCapInt lowMask = (ONE_BCI << start) - 1u;
    const bitCapInt midMask = (ONE_BCI << oQubits) - 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < nMaxQPower; i += stride) {
        const bitCapInt low = i & lowMask;
        const bitCapInt mid = (i >> start) & midMask;
        const bitCapInt high = i >> (start + oQubits);
        out[i] = a[low | (high << start)] * b[mid];
    }
}

template <typename R>
void launchCompose(const cplx<R>* a, const cplx<R>* b, cplx<R>* out, bitCapInt nMaxQPower,
    bitLenInt start, bitLenInt oQubits, hipStream_t stream)
{
    hipLaunchKernelGGL((k_compose<R>), dim3(gridFor(nMaxQPower)), dim3(QA_BLOCK), 0, stream, a, b,
        out, nMaxQPower, start, oQubits);
}

template <typename R>
__global__ void k_dispose_slice(const cplx<R>* in, cplx<R>* out, bitCapInt remPower, bitLenInt start,
    bitLenInt length, bitCapInt slicePerm, cplx<R> scale)
{
    const bitCapInt lowMask = (ONE_BCI << start) - 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt r = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; r < remPower; r += stride) {
        const bitCapInt low = r & lowMask;
        const bitCapInt high = (r >> start) << (start + length);
        out[r] = scale * in[low | (slicePerm << start) | high];
    }
}

template <typename R>
void launchDisposeSlice(const cplx<R>* in, cplx<R>* out, bitCapInt remPower, bitLenInt start,
    bitLenInt length, bitCapInt slicePerm, cplx<R> scale, hipStream_t stream)
{
    hipLaunchKernelGGL((k_dispose_slice<R>), dim3(gridFor(remPower)), dim3(QA_BLOCK), 0, stream, in,
        out, remPower, start, length, slicePerm, scale);
}

template <typename R>
__global__ void k_gather_part(const cplx<R>* in, cplx<R>* dest, bitCapInt partPower, bitLenInt start,
    bitLenInt length, bitCapInt remIndex, cplx<R> scale)
{
    const bitCapInt lowMask = (ONE_BCI << start) - 1u;
    const bitCapInt low = remIndex & lowMask;
    const bitCapInt high = (remIndex >> start) << (start + length);
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt p = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; p < partPower; p += stride) {
        dest[p] = scale * in[low | (p << start) | high];
    }
}

template <typename R>
void launchGatherPart(const cplx<R>* in, cplx<R>* dest, bitCapInt partPower, bitLenInt start,
    bitLenInt length, bitCapInt remIndex, cplx<R> scale, hipStream_t stream)
{
    hipLaunchKernelGGL((k_gather_part<R>), dim3(gridFor(partPower)), dim3(QA_BLOCK), 0, stream, in,
        dest, partPower, start, length, remIndex, scale);
}

template <typename R>
__global__ void k_allocate_expand(const cplx<R>* in, cplx<R>* out, bitCapInt nMaxQPower,
    bitLenInt start, bitLenInt length)
{
    const bitCapInt lowMask = (ONE_BCI << start) - 1u;
    const bitCapInt midMask = (ONE_BCI << length) - 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < nMaxQPower; i += stride) {
        const bitCapInt low = i & lowMask;
        const bitCapInt mid = (i >> start) & midMask;
        const bitCapInt high = i >> (start + length);
        out[i] = mid ? cplx<R>(0, 0) : in[low | (high << start)];
    }
}

template <typename R>
void launchAllocateExpand(const cplx<R>* in, cplx<R>* out, bitCapInt nMaxQPower, bitLenInt start,
    bitLenInt length, hipStream_t stream)
{
    hipLaunchKernelGGL((k_allocate_expand<R>), dim3(gridFor(nMaxQPower)), dim3(QA_BLOCK), 0, stream,
        in, out, nMaxQPower, start, length);
}

template <typename R> __global__ void k_shuffle_swap(cplx<R>* aHigh, cplx<R>* bLow, bitCapInt half)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const cplx<R> t = aHigh[i];
        aHigh[i] = bLow[i];
        bLow[i] = t;
    }
}

template <typename R>
void launchShuffleSwap(cplx<R>* aHigh, cplx<R>* bLow, bitCapInt half, hipStream_t stream)
{
    hipLaunchKernelGGL(
        (k_shuffle_swap<R>), dim3(gridFor(half)), dim3(QA_BLOCK), 0, stream, aHigh, bLow, half);
}

// ---- ALU / permutation ---------------------------------------------------------

__device__ __forceinline__ bitCapInt devModMul(bitCapInt a, bitCapInt b, bitCapInt m)
{
    return (bitCapInt)(((__uint128_t)a * b) % m);
}

__device__ __forceinline__ bitCapInt devModPow(bitCapInt base, bitCapInt e, bitCapInt m)
{
    bitCapInt result = 1u % m;
    base %= m;
    while (e) {
        if (e & 1u) result = devModMul(result, base, m);
        base = devModMul(base, base, m);
        e >>= 1u;
    }
    return result;
}

__device__ __forceinline__ bitCapInt tableRead(
    const unsigned char* table, bitCapInt entry, int bytes)
{
    bitCapInt v = 0;
    for (int b = 0; b < bytes; ++b) v |= ((bitCapInt)table[entry * bytes + b]) << (8 * b);
    return v;
}

template <typename R> __global__ void k_permute(const cplx<R>* sv, cplx<R>* nsv, PermArgs a)
{
    const bitCapInt lenMask = (ONE_BCI << a.length) - 1u;
    const bitCapInt regMask = lenMask << a.start;
    const bitCapInt lenPower = ONE_BCI << a.length;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < a.maxI; j += stride) {
        bitCapInt i = expandBits(j, a.qPowers, a.nPowers) | a.controlMask;
        const bitCapInt reg = (i & regMask) >> a.start;
        switch ((PermOp)a.op) {
        case PermOp::INC: {
            nsv[(i & ~regMask) | (((reg + a.operand) & lenMask) << a.start)] = sv[i];
            break;
        }
        case PermOp::INCDECC: {
            const bitCapInt out = reg + a.operand;
            const bitCapInt res = (out < lenPower)
                ? ((i & ~regMask) | (out << a.start))
                : ((i & ~regMask) | ((out - lenPower) << a.start) | a.carryMask);
            nsv[res] = sv[i];
            break;
        }
        case PermOp::INCS: {
            const bitCapInt out = (reg + a.operand) & lenMask;
            const bitCapInt signBit = ONE_BCI << (a.length - 1u);
            const bool ovf = (~(reg ^ a.operand) & (reg ^ out) & signBit) != 0;
            bitCapInt res = (i & ~regMask) | (out << a.start);
            if (ovf) res ^= a.carryMask;
            nsv[res] = sv[i];
            break;
        }
        case PermOp::MUL:
        case PermOp::DIV: {
            const bitCapInt carryRegMask = lenMask << a.start2;
            const bitCapInt out = reg * a.operand;
            const bitCapInt mapped = (i & ~(regMask | carryRegMask)) |
                ((out & lenMask) << a.start) | (((out >> a.length) & lenMask) << a.start2);
            if ((PermOp)a.op == PermOp::MUL) {
                nsv[mapped] = sv[i];
            } else {
                nsv[i] = sv[mapped];
            }
            break;
        }
        case PermOp::MULMODN:
        case PermOp::IMULMODN: {
            const bitCapInt outMask = ((ONE_BCI << a.length2) - 1u) << a.start2;
            const bitCapInt out = devModMul(reg, a.operand, a.modN);
            const bitCapInt mapped = (i & ~outMask) | (out << a.start2);
            if ((PermOp)a.op == PermOp::MULMODN) {
                nsv[mapped] = sv[i];
            } else {
                nsv[i] = sv[mapped];
            }
            break;
        }
        case PermOp::POWMODN: {
            const bitCapInt outMask = ((ONE_BCI << a.length2) - 1u) << a.start2;
            const bitCapInt out = devModPow(a.operand, reg, a.modN);
            nsv[(i & ~outMask) | (out << a.start2)] = sv[i];
            break;
        }
        case PermOp::HASH: {
            const bitCapInt val = tableRead(a.table, reg, a.tableBytes) & lenMask;
            nsv[(i & ~regMask) | (val << a.start)] = sv[i];
            break;
        }
        case PermOp::LDA: {
            // a.start/a.length = index register; a.start2/length2 = value register
            const bitCapInt idx = reg;
            const bitCapInt valMask = ((ONE_BCI << a.length2) - 1u) << a.start2;
            const bitCapInt val =
                tableRead(a.table, idx, a.tableBytes) & ((ONE_BCI << a.length2) - 1u);
            nsv[(i & ~valMask) | (val << a.start2)] = sv[i];
            break;
        }
        case PermOp::ADC:
        case PermOp::SBC: {
            const bitCapInt idx = reg;
            const bitCapInt valPower = ONE_BCI << a.length2;
            const bitCapInt valMask = (valPower - 1u) << a.start2;
            const bitCapInt tval = tableRead(a.table, idx, a.tableBytes) & (valPower - 1u);
            const bitCapInt val = (i & valMask) >> a.start2;
            bitCapInt out;
            if ((PermOp)a.op == PermOp::ADC) {
                out = val + tval + a.extra;
            } else {
                out = val + valPower - tval + a.extra;
            }
            const bitCapInt wrapped = out & (valPower - 1u);
            bitCapInt res = (i & ~valMask) | (wrapped << a.start2);
            if (out >= valPower) res |= a.carryMask;
            nsv[res] = sv[i];
            break;
        }
        case PermOp::INCBCD: {
            const int digits = (int)(a.length / 4u);
            bitCapInt value = 0, mul = 1, tenPow = 1;
            bool valid = true;
            for (int d = 0; d < digits; ++d) {
                const bitCapInt digit = (reg >> (4 * d)) & 0xFu;
                if (digit > 9u) valid = false;
                value += digit * mul;
                mul *= 10u;
                tenPow *= 10u;
            }
            if (!valid) {
                nsv[i] = sv[i];
                break;
            }
            bitCapInt out = (value + a.operand) % tenPow;
            bitCapInt enc = 0;
            for (int d = 0; d < digits; ++d) {
                enc |= (out % 10u) << (4 * d);
                out /= 10u;
            }
            nsv[(i & ~regMask) | (enc << a.start)] = sv[i];
            break;
        }
        case PermOp::ROL: {
            const bitLenInt shift = (bitLenInt)a.operand;
            const bitCapInt nreg = ((reg << shift) | (reg >> (a.length - shift))) & lenMask;
            nsv[(i & ~regMask) | (nreg << a.start)] = sv[i];
            break;
        }
        }
    }
}

template <typename R>
void launchPermute(const cplx<R>* sv, cplx<R>* nsv, const PermArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL((k_permute<R>), dim3(gridFor(a.maxI)), dim3(QA_BLOCK), 0, stream, sv, nsv, a);
}

// start vector for the controlled multiply family: the state with the
// fully-controlled subspace cleared (k_permute then fills that subspace)
template <typename R>
__global__ void k_copy_uncontrolled(
    const cplx<R>* sv, cplx<R>* nsv, bitCapInt maxQPower, bitCapInt controlMask)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        nsv[i] = ((i & controlMask) == controlMask) ? cplx<R>(0, 0) : sv[i];
    }
}

template <typename R>
void launchCopyUncontrolled(
    const cplx<R>* sv, cplx<R>* nsv, bitCapInt maxQPower, bitCapInt controlMask, hipStream_t stream)
{
    hipLaunchKernelGGL((k_copy_uncontrolled<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream,
        sv, nsv, maxQPower, controlMask);
}

template <typename R>
__global__ void k_phaseflipless(cplx<R>* sv, bitCapInt maxQPower, bitCapInt greaterPerm,
    bitLenInt start, bitCapInt regMask, bitCapInt flagMask)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower; i += stride) {
        if ((!flagMask || (i & flagMask)) && (((i & regMask) >> start) < greaterPerm)) {
            sv[i] = cplx<R>(-1, 0) * sv[i];
        }
    }
}

template <typename R>
void launchPhaseFlipIfLess(cplx<R>* sv, bitCapInt maxQPower, bitCapInt greaterPerm, bitLenInt start,
    bitCapInt regMask, bitCapInt flagMask, hipStream_t stream)
{
    hipLaunchKernelGGL((k_phaseflipless<R>), dim3(gridFor(maxQPower)), dim3(QA_BLOCK), 0, stream, sv,
        maxQPower, greaterPerm, start, regMask, flagMask);
}

// ---- fused QFT phase ramp ------------------------------------------------------

__device__ __forceinline__ bitCapInt insertZeroBitDev(bitCapInt i, bitCapInt p)
{
    return ((i & ~(p - 1u)) << 1u) | (i & (p - 1u));
}

template <typename R> __device__ __forceinline__ void devSinCos(R t, R* s, R* c);
template <> __device__ __forceinline__ void devSinCos<float>(float t, float* s, float* c)
{
    __sincosf(t, s, c);
}
template <> __device__ __forceinline__ void devSinCos<double>(double t, double* s, double* c)
{
    sincos(t, s, c);
}

template <typename R>
__global__ void k_phase_ramp(
    cplx<R>* sv, bitCapInt maxI, bitCapInt condPow, bitLenInt rampStart, bitCapInt rampMask, R scale)
{
    // condPow != 0: iterate the condPow-set half (maxI = maxQPower/2 with the
    // bit inserted); condPow == 0: iterate everything (maxI = maxQPower)
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < maxI; j += stride) {
        bitCapInt i = j;
        if (condPow) i = (((j & ~(condPow - 1u)) << 1u) | (j & (condPow - 1u))) | condPow;
        const bitCapInt frac = (i >> rampStart) & rampMask;
        const R theta = scale * (R)frac;
        R s, c;
        devSinCos<R>(theta, &s, &c);
        sv[i] = cplx<R>{ c, s } * sv[i];
    }
}

// fp32 vectorized: two adjacent indices per lane via float4
__global__ void k_phase_ramp_v(cplx<float>* sv, bitCapInt maxI, bitCapInt condPow,
    bitLenInt rampStart, bitCapInt rampMask, float scale)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt half = maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
        const bitCapInt j = 2u * k;
        bitCapInt i = j;
        if (condPow) i = (((j & ~(condPow - 1u)) << 1u) | (j & (condPow - 1u))) | condPow;
        const bitCapInt i4 = i >> 1u;
        float4 v = sv4[i4];
        const bitCapInt f0 = (i >> rampStart) & rampMask;
        const bitCapInt f1 = ((i + 1u) >> rampStart) & rampMask;
        float s0, c0, s1, c1;
        __sincosf(scale * (float)f0, &s0, &c0);
        __sincosf(scale * (float)f1, &s1, &c1);
        const cplx<float> a{ v.x, v.y }, b{ v.z, v.w };
        const cplx<float> na = cplx<float>{ c0, s0 } * a;
        const cplx<float> nb = cplx<float>{ c1, s1 } * b;
        sv4[i4] = make_float4(na.re, na.im, nb.re, nb.im);
    }
}

template <typename R>
void launchPhaseRamp(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt rampBits,
    bitCapInt condPower, double scale, hipStream_t stream)
{
    const bitCapInt maxI = condPower ? (maxQPower >> 1u) : maxQPower;
    const bitCapInt rampMask = (ONE_BCI << rampBits) - 1u;
    if constexpr (std::is_same_v<R, float>) {
        if ((condPower == 0u || condPower >= 2u) && (maxI & 1u) == 0u && maxI >= 2u) {
            hipLaunchKernelGGL((k_phase_ramp_v), dim3(gridFor(maxI >> 1u)), dim3(QA_BLOCK), 0,
                stream, sv, maxI, condPower, rampStart, rampMask, (float)scale);
            return;
        }
    }
    hipLaunchKernelGGL((k_phase_ramp<R>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0, stream, sv,
        maxI, condPower, rampStart, rampMask, (R)scale);
}

// fully fused QFT column: H on bit t AND the column's phase ramp in ONE
// pass. POST (QFT): out1 *= e^{i*scale*frac} after H; PRE (IQFT): in1 *=
// e^{i*scale*frac} before H. frac depends only on the pair base's low bits,
// so both elements of a float4 share their own frac values.
template <typename R, bool PRE>
__global__ void k_qft_col(
    cplx<R>* sv, bitCapInt maxI, bitCapInt tPow, bitLenInt rampStart, bitCapInt rampMask, R scale)
{
    const R s = (R)0.70710678118654752440;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < maxI; j += stride) {
        const bitCapInt i = ((j & ~(tPow - 1u)) << 1u) | (j & (tPow - 1u));
        const bitCapInt frac = (i >> rampStart) & rampMask;
        R sn, cs;
        devSinCos<R>(scale * (R)frac, &sn, &cs);
        const cplx<R> f{ cs, sn };
        cplx<R> x = sv[i];
        cplx<R> y = sv[i | tPow];
        if (PRE) y = f * y;
        cplx<R> o0 = s * (x + y);
        cplx<R> o1 = s * (x - y);
        if (!PRE) o1 = f * o1;
        sv[i] = o0;
        sv[i | tPow] = o1;
    }
}

// fp32 vectorized: two adjacent pairs per lane (requires tPow >= 2)
template <bool PRE>
__global__ void k_qft_col_v(
    cplx<float>* sv, bitCapInt maxI, bitCapInt tPow, bitLenInt rampStart, bitCapInt rampMask,
    float scale)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float s = 0.70710678f;
    const bitCapInt half = maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
        const bitCapInt j = 2u * k;
        const bitCapInt i = ((j & ~(tPow - 1u)) << 1u) | (j & (tPow - 1u));
        const bitCapInt lo4 = i >> 1u;
        const bitCapInt hi4 = (i | tPow) >> 1u;
        float4 vlo = sv4[lo4];
        float4 vhi = sv4[hi4];
        float s0, c0, s1, c1;
        __sincosf(scale * (float)((i >> rampStart) & rampMask), &s0, &c0);
        __sincosf(scale * (float)(((i + 1u) >> rampStart) & rampMask), &s1, &c1);
        const cplx<float> f0{ c0, s0 }, f1{ c1, s1 };
        cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
        cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
        if (PRE) {
            y0 = f0 * y0;
            y1 = f1 * y1;
        }
        cplx<float> a0 = s * (x0 + y0), a1 = s * (x1 + y1);
        cplx<float> b0 = s * (x0 - y0), b1 = s * (x1 - y1);
        if (!PRE) {
            b0 = f0 * b0;
            b1 = f1 * b1;
        }
        sv4[lo4] = make_float4(a0.re, a0.im, a1.re, a1.im);
        sv4[hi4] = make_float4(b0.re, b0.im, b1.re, b1.im);
    }
}

// generalized fused column: the ramp's bits may be relocated (distributed
// pager lazy qubit maps) — frac(i) = ((i >> rampStart) & inPlaceRelMask) +
// sum_k (i & sPow[k] ? sWeight[k] : 0), plus a constant phase0 (the
// meta-page scalar term folded into the same pass).
template <typename R, bool PRE>
__global__ void k_qft_col_gen(cplx<R>* sv, bitCapInt maxI, bitCapInt tPow, RampArgs a, R phase0)
{
    const R s = (R)0.70710678118654752440;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < maxI; j += stride) {
        const bitCapInt i = ((j & ~(tPow - 1u)) << 1u) | (j & (tPow - 1u));
        uint64_t frac = (uint64_t)((i >> a.rampStart) & a.inPlaceRelMask);
        for (int k = 0; k < a.nScattered; ++k) {
            if (i & a.sPow[k]) frac += a.sWeight[k];
        }
        R sn, cs;
        devSinCos<R>((R)a.scale * (R)frac + phase0, &sn, &cs);
        const cplx<R> f{ cs, sn };
        cplx<R> x = sv[i];
        cplx<R> y = sv[i | tPow];
        if (PRE) y = f * y;
        cplx<R> o0 = s * (x + y);
        cplx<R> o1 = s * (x - y);
        if (!PRE) o1 = f * o1;
        sv[i] = o0;
        sv[i | tPow] = o1;
    }
}

template <bool PRE>
__global__ void k_qft_col_gen_v(
    cplx<float>* sv, bitCapInt maxI, bitCapInt tPow, RampArgs a, float phase0)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float s = 0.70710678f;
    const bitCapInt half = maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < half; k += stride) {
        const bitCapInt j = 2u * k;
        const bitCapInt i = ((j & ~(tPow - 1u)) << 1u) | (j & (tPow - 1u));
        const bitCapInt lo4 = i >> 1u;
        const bitCapInt hi4 = (i | tPow) >> 1u;
        float4 vlo = sv4[lo4];
        float4 vhi = sv4[hi4];
        uint64_t fr0 = (uint64_t)((i >> a.rampStart) & a.inPlaceRelMask);
        uint64_t fr1 = (uint64_t)(((i + 1u) >> a.rampStart) & a.inPlaceRelMask);
        for (int t = 0; t < a.nScattered; ++t) {
            if (i & a.sPow[t]) fr0 += a.sWeight[t];
            if ((i + 1u) & a.sPow[t]) fr1 += a.sWeight[t];
        }
        float s0, c0, s1, c1;
        __sincosf((float)a.scale * (float)fr0 + phase0, &s0, &c0);
        __sincosf((float)a.scale * (float)fr1 + phase0, &s1, &c1);
        const cplx<float> f0{ c0, s0 }, f1{ c1, s1 };
        cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
        cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
        if (PRE) {
            y0 = f0 * y0;
            y1 = f1 * y1;
        }
        cplx<float> a0 = s * (x0 + y0), a1 = s * (x1 + y1);
        cplx<float> b0 = s * (x0 - y0), b1 = s * (x1 - y1);
        if (!PRE) {
            b0 = f0 * b0;
            b1 = f1 * b1;
        }
        sv4[lo4] = make_float4(a0.re, a0.im, a1.re, a1.im);
        sv4[hi4] = make_float4(b0.re, b0.im, b1.re, b1.im);
    }
}

// A/B experiment (QRACK_GPU_QFT_PIPE=1): software-pipelined column — loads
// for iteration i+1 issue before iteration i's stores, hiding the RMW
// turnaround on the two streams. Same math as k_qft_col_v<false>.
template <bool PRE>
__global__ void k_qft_col_v_pipe(
    cplx<float>* sv, bitCapInt maxI, bitCapInt tPow, bitLenInt rampStart, bitCapInt rampMask,
    float scale)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float s = 0.70710678f;
    const bitCapInt half = maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    bitCapInt kIt = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x;
    if (kIt >= half) return;
    auto idx = [&](bitCapInt kk, bitCapInt& lo4, bitCapInt& hi4, bitCapInt& i) {
        const bitCapInt j = 2u * kk;
        i = ((j & ~(tPow - 1u)) << 1u) | (j & (tPow - 1u));
        lo4 = i >> 1u;
        hi4 = (i | tPow) >> 1u;
    };
    bitCapInt lo4, hi4, i;
    idx(kIt, lo4, hi4, i);
    float4 vlo = sv4[lo4];
    float4 vhi = sv4[hi4];
    while (true) {
        const bitCapInt kNext = kIt + stride;
        bitCapInt nlo4 = 0, nhi4 = 0, ni = 0;
        float4 nlo{}, nhi{};
        const bool more = kNext < half;
        if (more) {
            idx(kNext, nlo4, nhi4, ni);
            nlo = sv4[nlo4]; // prefetch next pair before this one's stores
            nhi = sv4[nhi4];
        }
        float s0, c0, s1, c1;
        __sincosf(scale * (float)((i >> rampStart) & rampMask), &s0, &c0);
        __sincosf(scale * (float)(((i + 1u) >> rampStart) & rampMask), &s1, &c1);
        const cplx<float> f0{ c0, s0 }, f1{ c1, s1 };
        cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
        cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
        if (PRE) {
            y0 = f0 * y0;
            y1 = f1 * y1;
        }
        cplx<float> a0 = s * (x0 + y0), a1 = s * (x1 + y1);
        cplx<float> b0 = s * (x0 - y0), b1 = s * (x1 - y1);
        if (!PRE) {
            b0 = f0 * b0;
            b1 = f1 * b1;
        }
        sv4[lo4] = make_float4(a0.re, a0.im, a1.re, a1.im);
        sv4[hi4] = make_float4(b0.re, b0.im, b1.re, b1.im);
        if (!more) break;
        kIt = kNext;
        lo4 = nlo4;
        hi4 = nhi4;
        i = ni;
        vlo = nlo;
        vhi = nhi;
    }
}

template <typename R>
void launchQftColumnGeneral(cplx<R>* sv, bitCapInt maxQPower, bitCapInt tPow, const RampArgs& a,
    double phase0, bool pre, hipStream_t stream)
{
    const bitCapInt maxI = maxQPower >> 1u;
    if constexpr (std::is_same_v<R, float>) {
        if (tPow >= 2u && (maxI & 1u) == 0u) {
            if (pre) {
                hipLaunchKernelGGL((k_qft_col_gen_v<true>), dim3(gridFor(maxI >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, maxI, tPow, a, (float)phase0);
            } else {
                hipLaunchKernelGGL((k_qft_col_gen_v<false>), dim3(gridFor(maxI >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, maxI, tPow, a, (float)phase0);
            }
            return;
        }
    }
    if (pre) {
        hipLaunchKernelGGL((k_qft_col_gen<R, true>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0,
            stream, sv, maxI, tPow, a, (R)phase0);
    } else {
        hipLaunchKernelGGL((k_qft_col_gen<R, false>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0,
            stream, sv, maxI, tPow, a, (R)phase0);
    }
}

// TWO disjoint 4x4 gates per full-state pass (see kernels.hpp
// Gate4x4Pair2Args): each thread owns a 16-amplitude orbit over the two
// gates' four bit positions, applies gate A across its axis pair then
// gate B across the other — one state read+write for two SU(4)s.
template <typename R>
__global__ void __launch_bounds__(256, 3) k_mtrx2q_pair2(cplx<R>* sv, Gate4x4Pair2Args<R> a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < a.orbits;
         k += stride) {
        bitCapInt r = k;
        for (int b = 0; b < 4; ++b) r = insertZeroBitDev(r, a.sorted4[b]);
        bitCapInt idx[16];
        for (int ib = 0; ib < 4; ++ib) {
            for (int ia = 0; ia < 4; ++ia) {
                bitCapInt x = r;
                if (ia & 1) x |= a.pA1;
                if (ia & 2) x |= a.pA2;
                if (ib & 1) x |= a.pB1;
                if (ib & 2) x |= a.pB2;
                idx[4 * ib + ia] = x;
            }
        }
        cplx<R> v[16];
        for (int b = 0; b < 16; ++b) v[b] = sv[idx[b]];
        // gate A mixes the ia axis for each ib
        for (int ib = 0; ib < 4; ++ib) {
            cplx<R> out[4];
            for (int rI = 0; rI < 4; ++rI) {
                cplx<R> s(0, 0);
                for (int cI = 0; cI < 4; ++cI) s = s + a.mA[4 * rI + cI] * v[4 * ib + cI];
                out[rI] = s;
            }
            for (int rI = 0; rI < 4; ++rI) v[4 * ib + rI] = out[rI];
        }
        // gate B mixes the ib axis for each ia
        for (int ia = 0; ia < 4; ++ia) {
            cplx<R> out[4];
            for (int rI = 0; rI < 4; ++rI) {
                cplx<R> s(0, 0);
                for (int cI = 0; cI < 4; ++cI) s = s + a.mB[4 * rI + cI] * v[4 * cI + ia];
                out[rI] = s;
            }
            for (int rI = 0; rI < 4; ++rI) v[4 * rI + ia] = out[rI];
        }
        for (int b = 0; b < 16; ++b) sv[idx[b]] = v[b];
    }
}

template <typename R>
void launchMtrx2qPair2(cplx<R>* sv, const Gate4x4Pair2Args<R>& a, hipStream_t stream)
{
    hipLaunchKernelGGL(
        (k_mtrx2q_pair2<R>), dim3(gridFor(a.orbits)), dim3(QA_BLOCK), 0, stream, sv, a);
}

// TWO generalized QFT columns per pass for the distributed pager's local
// ladder: targets at ARBITRARY local slots (tPowHi/tPowLo by ROLE, not
// numeric order), ramp bits possibly relocated (RampArgs, which must
// EXCLUDE the low column's target bit — its contribution is the constant
// A = e^{i·sign·π/2}); per-column meta-page scalars phase0Hi/phase0Lo.
// Same algebra as k_qft_col2: f_hi(bLo) = f0·A^bLo·e^{i·phase0Hi},
// f_lo = f0²·e^{i·phase0Lo} with ONE sincos per orbit.
template <typename R, bool PRE>
__global__ void k_qft_col2_gen(cplx<R>* sv, bitCapInt orbits, bitCapInt tPowHi, bitCapInt tPowLo,
    RampArgs a, R phase0Hi, R phase0Lo)
{
    const R s = (R)0.70710678118654752440;
    const R iSign = (a.scale >= 0) ? (R)1 : (R)-1;
    const bitCapInt pLow = (tPowHi < tPowLo) ? tPowHi : tPowLo;
    const bitCapInt pHigh = (tPowHi < tPowLo) ? tPowLo : tPowHi;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < orbits;
         k += stride) {
        const bitCapInt r = insertZeroBitDev(insertZeroBitDev(k, pLow), pHigh);
        uint64_t frac = (uint64_t)((r >> a.rampStart) & a.inPlaceRelMask);
        for (int t = 0; t < a.nScattered; ++t) {
            if (r & a.sPow[t]) frac += a.sWeight[t];
        }
        R sn, cs;
        devSinCos<R>((R)a.scale * (R)frac, &sn, &cs);
        const cplx<R> f0{ cs, sn };
        const cplx<R> A{ 0, iSign };
        R snh, csh, snl, csl;
        devSinCos<R>(phase0Hi, &snh, &csh);
        devSinCos<R>(phase0Lo, &snl, &csl);
        const cplx<R> fHi0 = f0 * cplx<R>{ csh, snh };
        const cplx<R> fHi1 = fHi0 * A;
        const cplx<R> fLo = f0 * f0 * cplx<R>{ csl, snl };
        cplx<R> a00 = sv[r];
        cplx<R> a01 = sv[r | tPowLo];
        cplx<R> a10 = sv[r | tPowHi];
        cplx<R> a11 = sv[r | tPowHi | tPowLo];
        if (!PRE) {
            cplx<R> b00 = s * (a00 + a10), b01 = s * (a01 + a11);
            cplx<R> b10 = fHi0 * (s * (a00 - a10)), b11 = fHi1 * (s * (a01 - a11));
            sv[r] = s * (b00 + b01);
            sv[r | tPowLo] = fLo * (s * (b00 - b01));
            sv[r | tPowHi] = s * (b10 + b11);
            sv[r | tPowHi | tPowLo] = fLo * (s * (b10 - b11));
        } else {
            a01 = fLo * a01;
            a11 = fLo * a11;
            cplx<R> b00 = s * (a00 + a01), b01 = s * (a00 - a01);
            cplx<R> b10 = s * (a10 + a11), b11 = s * (a10 - a11);
            b10 = fHi0 * b10;
            b11 = fHi1 * b11;
            sv[r] = s * (b00 + b10);
            sv[r | tPowHi] = s * (b00 - b10);
            sv[r | tPowLo] = s * (b01 + b11);
            sv[r | tPowHi | tPowLo] = s * (b01 - b11);
        }
    }
}

template <typename R>
void launchQftColumn2General(cplx<R>* sv, bitCapInt maxQPower, bitCapInt tPowHi, bitCapInt tPowLo,
    const RampArgs& a, double phase0Hi, double phase0Lo, bool pre, hipStream_t stream)
{
    const bitCapInt orbits = maxQPower >> 2u;
    if (pre) {
        hipLaunchKernelGGL((k_qft_col2_gen<R, true>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tPowHi, tPowLo, a, (R)phase0Hi, (R)phase0Lo);
    } else {
        hipLaunchKernelGGL((k_qft_col2_gen<R, false>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tPowHi, tPowLo, a, (R)phase0Hi, (R)phase0Lo);
    }
}

// Ranged top-target fused column with receive-buffer fusion (pipelined
// distributed page exchange; see kernels.hpp). Pair rows r in [itLo, itHi):
//   x (target=0 side) = recvIsLow ? recvSrc[r-itLo] : sv[r]
//   y (target=1 side) = recvIsLow ? sv[r|tPow]      : recvSrc[r-itLo]
// outputs written in place to sv[r], sv[r|tPow]. Because the target is the
// TOP bit, the ramp fraction depends only on r (< tPow) and the pair map is
// the identity — no bit interleave needed.
template <typename R, bool PRE, bool RECV_LOW>
__global__ void k_qft_col_top_range(cplx<R>* sv, bitCapInt tPow, RampArgs a, R phase0,
    bitCapInt itLo, bitCapInt itHi, const cplx<R>* __restrict__ recvSrc)
{
    const R s = (R)0.70710678118654752440;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt r = itLo + (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; r < itHi;
         r += stride) {
        uint64_t frac = (uint64_t)((r >> a.rampStart) & a.inPlaceRelMask);
        for (int k = 0; k < a.nScattered; ++k) {
            if (r & a.sPow[k]) frac += a.sWeight[k];
        }
        R sn, cs;
        devSinCos<R>((R)a.scale * (R)frac + phase0, &sn, &cs);
        const cplx<R> f{ cs, sn };
        cplx<R> x = RECV_LOW ? recvSrc[r - itLo] : sv[r];
        cplx<R> y = RECV_LOW ? sv[r | tPow] : recvSrc[r - itLo];
        if (PRE) y = f * y;
        cplx<R> o0 = s * (x + y);
        cplx<R> o1 = s * (x - y);
        if (!PRE) o1 = f * o1;
        sv[r] = o0;
        sv[r | tPow] = o1;
    }
}

// float4-vectorized variant: two adjacent pair rows per thread (requires
// even itLo/itHi, which the chunking always produces for qpp >= 2)
template <bool PRE, bool RECV_LOW>
__global__ void k_qft_col_top_range_v(cplx<float>* sv, bitCapInt tPow, RampArgs a, float phase0,
    bitCapInt itLo, bitCapInt itHi, const cplx<float>* __restrict__ recvSrc)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float4* rc4 = reinterpret_cast<const float4*>(recvSrc);
    const float s = 0.70710678f;
    const bitCapInt lo4 = itLo >> 1u, hi4 = itHi >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = lo4 + (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < hi4;
         k += stride) {
        const bitCapInt r = 2u * k;
        const bitCapInt t4 = (r | tPow) >> 1u;
        float4 vlo = RECV_LOW ? rc4[k - lo4] : sv4[k];
        float4 vhi = RECV_LOW ? sv4[t4] : rc4[k - lo4];
        uint64_t fr0 = (uint64_t)((r >> a.rampStart) & a.inPlaceRelMask);
        uint64_t fr1 = (uint64_t)(((r + 1u) >> a.rampStart) & a.inPlaceRelMask);
        for (int t = 0; t < a.nScattered; ++t) {
            if (r & a.sPow[t]) fr0 += a.sWeight[t];
            if ((r + 1u) & a.sPow[t]) fr1 += a.sWeight[t];
        }
        float s0, c0, s1, c1;
        __sincosf((float)a.scale * (float)fr0 + phase0, &s0, &c0);
        __sincosf((float)a.scale * (float)fr1 + phase0, &s1, &c1);
        const cplx<float> f0{ c0, s0 }, f1{ c1, s1 };
        cplx<float> x0{ vlo.x, vlo.y }, x1{ vlo.z, vlo.w };
        cplx<float> y0{ vhi.x, vhi.y }, y1{ vhi.z, vhi.w };
        if (PRE) {
            y0 = f0 * y0;
            y1 = f1 * y1;
        }
        cplx<float> a0 = s * (x0 + y0), a1 = s * (x1 + y1);
        cplx<float> b0 = s * (x0 - y0), b1 = s * (x1 - y1);
        if (!PRE) {
            b0 = f0 * b0;
            b1 = f1 * b1;
        }
        sv4[k] = make_float4(a0.re, a0.im, a1.re, a1.im);
        sv4[t4] = make_float4(b0.re, b0.im, b1.re, b1.im);
    }
}

template <typename R>
void launchQftColumnTopRange(cplx<R>* sv, bitCapInt maxQPower, const RampArgs& a, double phase0,
    bool pre, bitCapInt itLo, bitCapInt itHi, const cplx<R>* recvSrc, bool recvIsLow,
    hipStream_t stream)
{
    const bitCapInt tPow = maxQPower >> 1u;
    const bitCapInt n = itHi - itLo;
    if (!n) return;
    if constexpr (std::is_same_v<R, float>) {
        if ((itLo & 1u) == 0u && (itHi & 1u) == 0u) {
            const dim3 g(gridFor(n >> 1u)), b(QA_BLOCK);
            if (pre) {
                if (recvIsLow)
                    hipLaunchKernelGGL((k_qft_col_top_range_v<true, true>), g, b, 0, stream, sv,
                        tPow, a, (float)phase0, itLo, itHi, recvSrc);
                else
                    hipLaunchKernelGGL((k_qft_col_top_range_v<true, false>), g, b, 0, stream, sv,
                        tPow, a, (float)phase0, itLo, itHi, recvSrc);
            } else {
                if (recvIsLow)
                    hipLaunchKernelGGL((k_qft_col_top_range_v<false, true>), g, b, 0, stream, sv,
                        tPow, a, (float)phase0, itLo, itHi, recvSrc);
                else
                    hipLaunchKernelGGL((k_qft_col_top_range_v<false, false>), g, b, 0, stream, sv,
                        tPow, a, (float)phase0, itLo, itHi, recvSrc);
            }
            return;
        }
    }
    const dim3 g(gridFor(n)), b(QA_BLOCK);
    if (pre) {
        if (recvIsLow)
            hipLaunchKernelGGL((k_qft_col_top_range<R, true, true>), g, b, 0, stream, sv, tPow, a,
                (R)phase0, itLo, itHi, recvSrc);
        else
            hipLaunchKernelGGL((k_qft_col_top_range<R, true, false>), g, b, 0, stream, sv, tPow,
                a, (R)phase0, itLo, itHi, recvSrc);
    } else {
        if (recvIsLow)
            hipLaunchKernelGGL((k_qft_col_top_range<R, false, true>), g, b, 0, stream, sv, tPow,
                a, (R)phase0, itLo, itHi, recvSrc);
        else
            hipLaunchKernelGGL((k_qft_col_top_range<R, false, false>), g, b, 0, stream, sv, tPow,
                a, (R)phase0, itLo, itHi, recvSrc);
    }
}

// TWO QFT columns fused in ONE full-state pass (halves the pass count of
// the already-fused per-column ladder): columns (col, col-1) process
// 4-amplitude orbits over bits (tHi, tLo). The cross-column ramp term is a
// CONSTANT factor iF = e^{i·sign·π/2} and the lower column's ramp is the
// square of the upper's, so ONE sincos per orbit drives all three phase
// factors:  f_hi(bLo) = f0·iF^bLo,  f_lo = f0².
// Forward (PRE=false, QFT): H_hi, ramp_hi, H_lo, ramp_lo.
// Inverse (PRE=true, IQFT): ramp_lo, H_lo, ramp_hi, H_hi (exact adjoint).
template <typename R, bool PRE>
__global__ void k_qft_col2(cplx<R>* sv, bitCapInt orbits, bitCapInt tHi, bitCapInt tLo,
    bitLenInt rampStart, bitCapInt lowMask, R scaleHi)
{
    const R s = (R)0.70710678118654752440;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    // iF = e^{i·sign·π/2}; sign is carried in scaleHi's sign
    const R iSign = (scaleHi >= 0) ? (R)1 : (R)-1;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < orbits;
         k += stride) {
        const bitCapInt r = insertZeroBitDev(insertZeroBitDev(k, tLo), tHi);
        const uint64_t lf = (uint64_t)((r >> rampStart) & lowMask);
        R sn, cs;
        devSinCos<R>(scaleHi * (R)lf, &sn, &cs);
        const cplx<R> f0{ cs, sn };
        const cplx<R> iF{ 0, iSign };
        const cplx<R> fHi0 = f0, fHi1 = f0 * iF;
        const cplx<R> fLo = f0 * f0;
        cplx<R> a00 = sv[r];
        cplx<R> a01 = sv[r | tLo];
        cplx<R> a10 = sv[r | tHi];
        cplx<R> a11 = sv[r | tHi | tLo];
        if (!PRE) {
            // H_hi then ramp_hi (phase on bHi=1, depends on bLo)
            cplx<R> b00 = s * (a00 + a10), b01 = s * (a01 + a11);
            cplx<R> b10 = fHi0 * (s * (a00 - a10)), b11 = fHi1 * (s * (a01 - a11));
            // H_lo then ramp_lo (phase on bLo=1)
            sv[r] = s * (b00 + b01);
            sv[r | tLo] = fLo * (s * (b00 - b01));
            sv[r | tHi] = s * (b10 + b11);
            sv[r | tHi | tLo] = fLo * (s * (b10 - b11));
        } else {
            // ramp_lo then H_lo
            a01 = fLo * a01;
            a11 = fLo * a11;
            cplx<R> b00 = s * (a00 + a01), b01 = s * (a00 - a01);
            cplx<R> b10 = s * (a10 + a11), b11 = s * (a10 - a11);
            // ramp_hi then H_hi
            b10 = fHi0 * b10;
            b11 = fHi1 * b11;
            sv[r] = s * (b00 + b10);
            sv[r | tHi] = s * (b00 - b10);
            sv[r | tLo] = s * (b01 + b11);
            sv[r | tHi | tLo] = s * (b01 - b11);
        }
    }
}

// float4-vectorized: each thread drives TWO adjacent orbits (8 amplitudes,
// 4 float4 RMWs). Requires tLo >= 2.
template <bool PRE>
__global__ void k_qft_col2_v(cplx<float>* sv, bitCapInt orbitPairs, bitCapInt tHi, bitCapInt tLo,
    bitLenInt rampStart, bitCapInt lowMask, float scaleHi)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float s = 0.70710678f;
    const float iSign = (scaleHi >= 0) ? 1.0f : -1.0f;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt m = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; m < orbitPairs;
         m += stride) {
        const bitCapInt r = insertZeroBitDev(insertZeroBitDev(2u * m, tLo), tHi);
        const bitCapInt i00 = r >> 1u;
        const bitCapInt i01 = (r | tLo) >> 1u;
        const bitCapInt i10 = (r | tHi) >> 1u;
        const bitCapInt i11 = (r | tHi | tLo) >> 1u;
        float4 v00 = sv4[i00], v01 = sv4[i01], v10 = sv4[i10], v11 = sv4[i11];
        const uint64_t lf0 = (uint64_t)((r >> rampStart) & lowMask);
        const uint64_t lf1 = (uint64_t)(((r + 1u) >> rampStart) & lowMask);
        float s0, c0, s1, c1;
        __sincosf(scaleHi * (float)lf0, &s0, &c0);
        __sincosf(scaleHi * (float)lf1, &s1, &c1);
        const cplx<float> f0a{ c0, s0 }, f0b{ c1, s1 };
        const cplx<float> iF{ 0.0f, iSign };
#define QA_COL2_BODY(aA, aB, aC, aD, f0)                                                           \
    {                                                                                              \
        const cplx<float> fHi0 = f0, fHi1 = f0 * iF, fLo = f0 * f0;                                \
        if (!PRE) {                                                                                \
            cplx<float> b00 = s * (aA + aC), b01 = s * (aB + aD);                                  \
            cplx<float> b10 = fHi0 * (s * (aA - aC)), b11 = fHi1 * (s * (aB - aD));                \
            aA = s * (b00 + b01);                                                                  \
            aB = fLo * (s * (b00 - b01));                                                          \
            aC = s * (b10 + b11);                                                                  \
            aD = fLo * (s * (b10 - b11));                                                          \
        } else {                                                                                   \
            cplx<float> t01 = fLo * aB, t11 = fLo * aD;                                            \
            cplx<float> b00 = s * (aA + t01), b01 = s * (aA - t01);                                \
            cplx<float> b10 = s * (aC + t11), b11 = s * (aC - t11);                                \
            b10 = fHi0 * b10;                                                                      \
            b11 = fHi1 * b11;                                                                      \
            aA = s * (b00 + b10);                                                                  \
            aC = s * (b00 - b10);                                                                  \
            aB = s * (b01 + b11);                                                                  \
            aD = s * (b01 - b11);                                                                  \
        }                                                                                          \
    }
        cplx<float> x00{ v00.x, v00.y }, y00{ v00.z, v00.w };
        cplx<float> x01{ v01.x, v01.y }, y01{ v01.z, v01.w };
        cplx<float> x10{ v10.x, v10.y }, y10{ v10.z, v10.w };
        cplx<float> x11{ v11.x, v11.y }, y11{ v11.z, v11.w };
        QA_COL2_BODY(x00, x01, x10, x11, f0a);
        QA_COL2_BODY(y00, y01, y10, y11, f0b);
#undef QA_COL2_BODY
        sv4[i00] = make_float4(x00.re, x00.im, y00.re, y00.im);
        sv4[i01] = make_float4(x01.re, x01.im, y01.re, y01.im);
        sv4[i10] = make_float4(x10.re, x10.im, y10.re, y10.im);
        sv4[i11] = make_float4(x11.re, x11.im, y11.re, y11.im);
    }
}

// THREE QFT columns fused per pass (8-amplitude orbits). Phase structure:
// with f0 = e^{i·s_hi·lf}, A = e^{i·sign·π/2} = ±i, B = e^{i·sign·π/4}:
//   ramp_hi(bMid,bLo) = f0·A^bMid·B^bLo, ramp_mid(bLo) = f0²·A^bLo,
//   ramp_lo = f0⁴ — still ONE sincos per orbit.
template <typename R, bool PRE>
__global__ void k_qft_col3(cplx<R>* sv, bitCapInt orbits, bitCapInt tHi, bitCapInt tMid,
    bitCapInt tLo, bitLenInt rampStart, bitCapInt lowMask, R scaleHi)
{
    const R s = (R)0.70710678118654752440;
    const R c45 = (R)0.70710678118654752440;
    const R iSign = (scaleHi >= 0) ? (R)1 : (R)-1;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < orbits;
         k += stride) {
        const bitCapInt r =
            insertZeroBitDev(insertZeroBitDev(insertZeroBitDev(k, tLo), tMid), tHi);
        bitCapInt idx[8];
        for (int b = 0; b < 8; ++b) {
            idx[b] = r | ((b & 4) ? tHi : 0u) | ((b & 2) ? tMid : 0u) | ((b & 1) ? tLo : 0u);
        }
        cplx<R> v[8];
        for (int b = 0; b < 8; ++b) v[b] = sv[idx[b]];
        const uint64_t lf = (uint64_t)((r >> rampStart) & lowMask);
        R sn, cs;
        devSinCos<R>(scaleHi * (R)lf, &sn, &cs);
        const cplx<R> f0{ cs, sn };
        const cplx<R> A{ 0, iSign };
        const cplx<R> B{ c45, iSign * c45 };
        const cplx<R> f2 = f0 * f0;
        const cplx<R> f4 = f2 * f2;
        // per-slot hi-ramp factors for bHi=1: f0 * A^bMid * B^bLo
        cplx<R> fh[4];
        fh[0] = f0;
        fh[1] = f0 * B;
        fh[2] = f0 * A;
        fh[3] = f0 * A * B;
        auto hPair = [&](int lo, int hi) {
            const cplx<R> t = s * (v[lo] + v[hi]);
            const cplx<R> u = s * (v[lo] - v[hi]);
            v[lo] = t;
            v[hi] = u;
        };
        if (!PRE) {
            for (int b = 0; b < 4; ++b) hPair(b, b | 4);
            for (int m = 0; m < 4; ++m) v[4 | m] = fh[m] * v[4 | m];
            hPair(0, 2);
            hPair(1, 3);
            hPair(4, 6);
            hPair(5, 7);
            v[2] = f2 * v[2];
            v[3] = f2 * A * v[3];
            v[6] = f2 * v[6];
            v[7] = f2 * A * v[7];
            hPair(0, 1);
            hPair(2, 3);
            hPair(4, 5);
            hPair(6, 7);
            v[1] = f4 * v[1];
            v[3] = f4 * v[3];
            v[5] = f4 * v[5];
            v[7] = f4 * v[7];
        } else {
            // exact adjoint order (angles carry the sign): ramp_lo, H_lo,
            // ramp_mid, H_mid, ramp_hi, H_hi
            v[1] = f4 * v[1];
            v[3] = f4 * v[3];
            v[5] = f4 * v[5];
            v[7] = f4 * v[7];
            hPair(0, 1);
            hPair(2, 3);
            hPair(4, 5);
            hPair(6, 7);
            v[2] = f2 * v[2];
            v[3] = f2 * A * v[3];
            v[6] = f2 * v[6];
            v[7] = f2 * A * v[7];
            hPair(0, 2);
            hPair(1, 3);
            hPair(4, 6);
            hPair(5, 7);
            for (int m = 0; m < 4; ++m) v[4 | m] = fh[m] * v[4 | m];
            for (int b = 0; b < 4; ++b) hPair(b, b | 4);
        }
        for (int b = 0; b < 8; ++b) sv[idx[b]] = v[b];
    }
}

// float4-vectorized 3-column kernel: two adjacent orbits per thread
// (16 amplitudes, 8 float4 RMWs); requires tLo >= 2.
template <bool PRE>
__global__ void k_qft_col3_v(cplx<float>* sv, bitCapInt orbitPairs, bitCapInt tHi, bitCapInt tMid,
    bitCapInt tLo, bitLenInt rampStart, bitCapInt lowMask, float scaleHi)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const float s = 0.70710678f;
    const float iSign = (scaleHi >= 0) ? 1.0f : -1.0f;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt m = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; m < orbitPairs;
         m += stride) {
        const bitCapInt r =
            insertZeroBitDev(insertZeroBitDev(insertZeroBitDev(2u * m, tLo), tMid), tHi);
        bitCapInt idx[8];
        for (int b = 0; b < 8; ++b) {
            idx[b] =
                (r | ((b & 4) ? tHi : 0u) | ((b & 2) ? tMid : 0u) | ((b & 1) ? tLo : 0u)) >> 1u;
        }
        float4 raw[8];
        for (int b = 0; b < 8; ++b) raw[b] = sv4[idx[b]];
        const uint64_t lf0 = (uint64_t)((r >> rampStart) & lowMask);
        const uint64_t lf1 = (uint64_t)(((r + 1u) >> rampStart) & lowMask);
        float s0, c0, s1, c1;
        __sincosf(scaleHi * (float)lf0, &s0, &c0);
        __sincosf(scaleHi * (float)lf1, &s1, &c1);
        const cplx<float> A{ 0.0f, iSign };
        const cplx<float> B{ 0.70710678f, iSign * 0.70710678f };
        for (int half = 0; half < 2; ++half) {
            const cplx<float> f0 = half ? cplx<float>{ c1, s1 } : cplx<float>{ c0, s0 };
            const cplx<float> f2 = f0 * f0;
            const cplx<float> f4 = f2 * f2;
            cplx<float> fh[4] = { f0, f0 * B, f0 * A, f0 * A * B };
            cplx<float> v[8];
            for (int b = 0; b < 8; ++b) {
                v[b] = half ? cplx<float>{ raw[b].z, raw[b].w } : cplx<float>{ raw[b].x, raw[b].y };
            }
            auto hPair = [&](int lo, int hi) {
                const cplx<float> t = s * (v[lo] + v[hi]);
                const cplx<float> u = s * (v[lo] - v[hi]);
                v[lo] = t;
                v[hi] = u;
            };
            if (!PRE) {
                for (int b = 0; b < 4; ++b) hPair(b, b | 4);
                for (int q = 0; q < 4; ++q) v[4 | q] = fh[q] * v[4 | q];
                hPair(0, 2);
                hPair(1, 3);
                hPair(4, 6);
                hPair(5, 7);
                v[2] = f2 * v[2];
                v[3] = f2 * A * v[3];
                v[6] = f2 * v[6];
                v[7] = f2 * A * v[7];
                hPair(0, 1);
                hPair(2, 3);
                hPair(4, 5);
                hPair(6, 7);
                v[1] = f4 * v[1];
                v[3] = f4 * v[3];
                v[5] = f4 * v[5];
                v[7] = f4 * v[7];
            } else {
                v[1] = f4 * v[1];
                v[3] = f4 * v[3];
                v[5] = f4 * v[5];
                v[7] = f4 * v[7];
                hPair(0, 1);
                hPair(2, 3);
                hPair(4, 5);
                hPair(6, 7);
                v[2] = f2 * v[2];
                v[3] = f2 * A * v[3];
                v[6] = f2 * v[6];
                v[7] = f2 * A * v[7];
                hPair(0, 2);
                hPair(1, 3);
                hPair(4, 6);
                hPair(5, 7);
                for (int q = 0; q < 4; ++q) v[4 | q] = fh[q] * v[4 | q];
                for (int b = 0; b < 4; ++b) hPair(b, b | 4);
            }
            for (int b = 0; b < 8; ++b) {
                if (half) {
                    raw[b].z = v[b].re;
                    raw[b].w = v[b].im;
                } else {
                    raw[b].x = v[b].re;
                    raw[b].y = v[b].im;
                }
            }
        }
        for (int b = 0; b < 8; ++b) sv4[idx[b]] = raw[b];
    }
}

// K-column orbit apply over 16 register-resident amplitudes — the same math
// as k_qft_colK (one f0 plus constant roots of unity drive every ramp), as a
// building block for the LDS-staged ladder kernels. v[b] is the amplitude
// whose group-column bits spell b; U[d] = e^{i·sign·π/2^d}; f0 encodes the
// below-group ramp contribution at the group's HIGHEST column scale.
template <typename R, int K, bool PRE>
__device__ __forceinline__ void qftOrbitColumns(cplx<R>* v, R iSign, cplx<R> f0)
{
    const R s = (R)0.70710678118654752440;
    constexpr int NS = 1 << K;
    // U(d) = e^{i·sign·π/2^d} — compile-time roots of unity (indices below
    // are constants after full unrolling, so these fold into immediates)
    const cplx<R> U[4] = { cplx<R>{ (R)1, (R)0 }, cplx<R>{ (R)0, iSign },
        cplx<R>{ (R)0.70710678118654752440, iSign * (R)0.70710678118654752440 },
        cplx<R>{ (R)0.92387953251128675613, iSign * (R)0.38268343236508977173 } };
    cplx<R> fPow[K];
    fPow[0] = f0;
#pragma unroll
    for (int m = 1; m < K; ++m) fPow[m] = fPow[m - 1] * fPow[m - 1];
    auto column = [&](int c) {
#pragma unroll
        for (int b = 0; b < NS; ++b) {
            if (b & (1 << c)) continue;
            const int hb = b | (1 << c);
            const cplx<R> t = s * (v[b] + v[hb]);
            const cplx<R> u = s * (v[b] - v[hb]);
            v[b] = t;
            v[hb] = u;
        }
#pragma unroll
        for (int b = 0; b < NS; ++b) {
            if (!(b & (1 << c))) continue;
            cplx<R> f = fPow[K - 1 - c];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (j < c && (b & (1 << j))) f = f * U[c - j];
            }
            v[b] = f * v[b];
        }
    };
    auto columnInv = [&](int c) {
#pragma unroll
        for (int b = 0; b < NS; ++b) {
            if (!(b & (1 << c))) continue;
            cplx<R> f = fPow[K - 1 - c];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (j < c && (b & (1 << j))) f = f * U[c - j];
            }
            v[b] = f * v[b];
        }
#pragma unroll
        for (int b = 0; b < NS; ++b) {
            if (b & (1 << c)) continue;
            const int hb = b | (1 << c);
            const cplx<R> t = s * (v[b] + v[hb]);
            const cplx<R> u = s * (v[b] - v[hb]);
            v[b] = t;
            v[hb] = u;
        }
    };
    if (!PRE) {
#pragma unroll
        for (int c = K - 1; c >= 0; --c) column(c);
    } else {
#pragma unroll
        for (int c = 0; c < K; ++c) columnInv(c);
    }
}

// LDS bank swizzle for the low-ladder kernel: XOR index bits 4..7 into
// bits 0..3 so every access pattern the orbit groups generate (element
// strides 1, 16, 256 within a wave) lands on 16 distinct bank pairs per
// 16 consecutive lanes — the optimum for 8/16-byte LDS elements.
__device__ __forceinline__ int qaSwz(int j) { return j ^ ((j >> 4) & 15); }

// Value barrier for a synthesised amplitude: the optimiser must treat it
// like a loaded one. Seeing the select, it folds the known zeros into the
// orbit arithmetic and contracts the rest into different FMAs than the
// normal kernel's, and the stores are then no longer bit-identical to it.
template <typename R> __device__ __forceinline__ cplx<R> qaOpaque(cplx<R> a)
{
    asm volatile("" : "+v"(a.re), "+v"(a.im));
    return a;
}

// Input of a support-restricted pass (QftSupportArgs) at global index x,
// *elem being sv[x]: the load is predicated, memory outside the support is
// never read.
template <typename R>
__device__ __forceinline__ cplx<R> qaSupportLoad(
    const cplx<R>* elem, bitCapInt x, const QftSupportArgs& sup, cplx<R> phase)
{
    cplx<R> a{ (R)0, (R)0 };
    if (((x ^ sup.perm) & sup.fixedMask) == 0u) a = sup.fromBuffer ? *elem : phase;
    return a;
}

// c-th active tile of a support-restricted pass: the bits of c deposited
// into the set bits of freeMask, lowest first, over the fixed bits
__device__ __forceinline__ bitCapInt qaSupportTile(bitCapInt c, bitCapInt freeMask, bitCapInt fixed)
{
    bitCapInt t = fixed;
    for (bitCapInt m = freeMask; m; m &= m - 1u, c >>= 1u) {
        if (c & 1u) t |= m & (~m + 1u);
    }
    return t;
}

// One group of K columns applied over a 2^tb-amplitude tile as 16-amp
// register orbits. K is a template parameter so v[] stays in registers
// (runtime K forces the array to scratch — measured 2.5x slower). Groups
// with gLo >= 6 may read/write HBM directly (lane-contiguous within the
// orbit slot loops); gLo < 6 groups always go through (swizzled) LDS.
//
// BASIS: the source is the basis state phase·|perm> and the buffer contents
// are undefined — a fromGlobal gather synthesises its values from the index
// (idxBase = the tile's first global index) instead of loading them; the
// arithmetic, zeros included, is unchanged. SUMS: a toGlobal scatter also
// adds the norm of every amplitude it stores into `acc`.
//
// MASKED: a support-restricted pass — the fromGlobal gather goes through
// qaSupportLoad (phase or a predicated load inside the support, +0 outside).
template <typename R, int K, bool PRE, bool BASIS = false, bool SUMS = false, bool MASKED = false>
__device__ __forceinline__ void qftLowGroup(cplx<R>* svBase, cplx<R>* lds, int tile, int gLo,
    R scaleHi, R iSign, bool fromGlobal, bool toGlobal, bitCapInt idxBase = 0u,
    bitCapInt perm = 0u, cplx<R> phase = cplx<R>{ (R)0, (R)0 }, double* acc = nullptr,
    const QftSupportArgs* sup = nullptr)
{
    constexpr int NS = 1 << K;
    const int orbitCount = tile >> K;
    for (int o = threadIdx.x; o < orbitCount; o += blockDim.x) {
        const int below = o & ((1 << gLo) - 1);
        const int r = ((o >> gLo) << (gLo + K)) | below;
        cplx<R> v[NS];
        if (fromGlobal) {
            if (MASKED) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    const int j = r | (b << gLo);
                    v[b] = qaOpaque<R>(
                        qaSupportLoad<R>(svBase + j, idxBase | (bitCapInt)j, *sup, phase));
                }
            } else if (BASIS) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    v[b] = qaOpaque<R>(((idxBase | (bitCapInt)(r | (b << gLo))) == perm)
                            ? phase
                            : cplx<R>{ (R)0, (R)0 });
                }
            } else {
#pragma unroll
                for (int b = 0; b < NS; ++b) v[b] = svBase[r | (b << gLo)];
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) v[b] = lds[qaSwz(r | (b << gLo))];
        }
        R sn, cs;
        devSinCos<R>(scaleHi * (R)below, &sn, &cs);
        qftOrbitColumns<R, K, PRE>(v, iSign, cplx<R>{ cs, sn });
        if (toGlobal) {
#pragma unroll
            for (int b = 0; b < NS; ++b) svBase[r | (b << gLo)] = v[b];
            if (SUMS) {
#pragma unroll
                for (int b = 0; b < NS; ++b) *acc += (double)norm(v[b]);
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) lds[qaSwz(r | (b << gLo))] = v[b];
        }
    }
}



// ALL low-bit QFT columns in ONE pass: when the register starts at bit 0,
// columns colMax..0 act entirely inside a contiguous 2^tb-amplitude tile.
// Columns are processed in groups of (up to) 4 as 16-amplitude register
// orbits — the first group gathers straight from HBM, the last scatters
// straight back, and LDS carries the tile between groups. One global
// read+write, 2 barriers, and 1 sincos per orbit per group replace the
// former per-pair sincos ladder. tb = 12 (fp32) / 11 (fp64).
template <typename R, int K, bool PRE>
__global__ void __launch_bounds__(256, 3)
    k_qft_low_lds(cplx<R>* sv, bitCapInt nTiles, int tb, int colMax, R piSign)
{
    // REQUIRES colMax+1 to be a multiple of K (the engine aligns the ladder
    // length; K = 4 fp32 / 3 fp64) so every group is the single kernel-wide
    // instantiation — keeps the orbit registers allocated without spills.
    extern __shared__ unsigned char qa_lds_raw[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw);
    const int tile = 1 << tb;
    const int nCols = colMax + 1;
    const int nG = nCols / K;
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    // a group may touch HBM directly only if its orbit slot loops are
    // lane-contiguous, i.e. gLo >= 6; otherwise a contiguous LDS<->HBM
    // copy brackets the ladder on that side
    const int firstG = PRE ? 0 : (nG - 1);
    const int lastG = PRE ? (nG - 1) : 0;
    const bool copyIn = (K * firstG) < 6;
    const bool copyOut = (K * lastG) < 6;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        cplx<R>* svBase = sv + (t << tb);
        if (copyIn) {
            for (int j = threadIdx.x; j < tile; j += blockDim.x) lds[qaSwz(j)] = svBase[j];
        }
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0) && !copyIn;
            const bool toGlobal = (gi == nG - 1) && !copyOut;
            const R scaleHi = piSign / (R)(1 << (gLo + K - 1));
            if (gi != 0 || copyIn) __syncthreads();
            qftLowGroup<R, K, PRE>(svBase, lds, tile, gLo, scaleHi, iSign, fromGlobal, toGlobal);
        }
        if (copyOut) {
            __syncthreads();
            for (int j = threadIdx.x; j < tile; j += blockDim.x) svBase[j] = lds[qaSwz(j)];
        }
        __syncthreads();
    }
}

// k_qft_low_lds with a synthesised source and/or a norm epilogue. The loop
// is the normal kernel's, repeated here rather than shared through a
// device function so the normal kernel compiles exactly as before.
// BASIS: first pass of a ladder whose source is the basis state
// phase·|perm> — the state is synthesised from the index instead of read
// (the buffer holds nothing defined yet); the stores are bit-identical to
// the normal kernel's. SUMS: also leaves tileSums[t] = sum of |amp|^2 over
// the 2^tb amplitudes of tile t, taken from the values it stores.
template <typename R, int K, bool PRE, bool BASIS, bool SUMS>
__global__ void __launch_bounds__(256, 3) k_qft_low_lds_var(cplx<R>* sv, bitCapInt nTiles, int tb,
    int colMax, R piSign, bitCapInt perm, cplx<R> phase, double* tileSums)
{
    // REQUIRES colMax+1 to be a multiple of K (the engine aligns the ladder
    // length; K = 4 fp32 / 3 fp64) so every group is the single kernel-wide
    // instantiation — keeps the orbit registers allocated without spills.
    extern __shared__ unsigned char qa_lds_raw[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw);
    const int tile = 1 << tb;
    const int nCols = colMax + 1;
    const int nG = nCols / K;
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    // a group may touch HBM directly only if its orbit slot loops are
    // lane-contiguous, i.e. gLo >= 6; otherwise a contiguous LDS<->HBM
    // copy brackets the ladder on that side
    const int firstG = PRE ? 0 : (nG - 1);
    const int lastG = PRE ? (nG - 1) : 0;
    const bool copyIn = (K * firstG) < 6;
    const bool copyOut = (K * lastG) < 6;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        cplx<R>* svBase = sv + (t << tb);
        const bitCapInt idxBase = t << tb;
        double acc = 0;
        if (copyIn) {
            if (BASIS) {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) {
                    lds[qaSwz(j)] =
                        ((idxBase | (bitCapInt)j) == perm) ? phase : cplx<R>{ (R)0, (R)0 };
                }
            } else {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) lds[qaSwz(j)] = svBase[j];
            }
        }
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0) && !copyIn;
            const bool toGlobal = (gi == nG - 1) && !copyOut;
            const R scaleHi = piSign / (R)(1 << (gLo + K - 1));
            if (gi != 0 || copyIn) __syncthreads();
            qftLowGroup<R, K, PRE, BASIS, SUMS>(svBase, lds, tile, gLo, scaleHi, iSign,
                fromGlobal, toGlobal, idxBase, perm, phase, &acc);
        }
        if (copyOut) {
            __syncthreads();
            if (SUMS) {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) {
                    const cplx<R> a = lds[qaSwz(j)];
                    svBase[j] = a;
                    acc += (double)norm(a);
                }
            } else {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) svBase[j] = lds[qaSwz(j)];
            }
        }
        if (SUMS) {
            // fixed-order block reduction: wave shuffle tree, then the
            // waves in index order — one double per tile, no atomics
            __shared__ double waveSums[QA_BLOCK / 64];
            acc = waveReduceSum(acc);
            if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double s = 0;
                for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += waveSums[w];
                tileSums[t] = s;
            }
        }
        __syncthreads();
    }
}

template <typename R>
void launchQftLowLds(
    cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, int sign, bool pre, hipStream_t stream)
{
    constexpr int K = qaLowLadderK<R>();
    const bitCapInt nTiles = maxQPower >> tb;
    const size_t ldsBytes = (size_t(1) << tb) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    const R piSign = (R)sign * (R)3.14159265358979323846;
    if (pre) {
        hipLaunchKernelGGL((k_qft_low_lds<R, K, true>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
            stream, sv, nTiles, tb, colMax, piSign);
    } else {
        hipLaunchKernelGGL((k_qft_low_lds<R, K, false>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
            stream, sv, nTiles, tb, colMax, piSign);
    }
}

template <typename R>
void launchQftLowLdsBasis(cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, int sign, bool pre,
    bitCapInt perm, cplx<R> phase, hipStream_t stream)
{
    constexpr int K = qaLowLadderK<R>();
    const bitCapInt nTiles = maxQPower >> tb;
    const size_t ldsBytes = (size_t(1) << tb) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    const R piSign = (R)sign * (R)3.14159265358979323846;
    if (pre) {
        hipLaunchKernelGGL((k_qft_low_lds_var<R, K, true, true, false>), dim3(grid),
            dim3(QA_BLOCK), ldsBytes, stream, sv, nTiles, tb, colMax, piSign, perm, phase,
            (double*)nullptr);
    } else {
        hipLaunchKernelGGL((k_qft_low_lds_var<R, K, false, true, false>), dim3(grid),
            dim3(QA_BLOCK), ldsBytes, stream, sv, nTiles, tb, colMax, piSign, perm, phase,
            (double*)nullptr);
    }
}

template <typename R>
void launchQftLowLdsSums(cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, double* tileSumsDev,
    hipStream_t stream)
{
    constexpr int K = qaLowLadderK<R>();
    const bitCapInt nTiles = maxQPower >> tb;
    const size_t ldsBytes = (size_t(1) << tb) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    const R piSign = (R)3.14159265358979323846;
    hipLaunchKernelGGL((k_qft_low_lds_var<R, K, false, false, true>), dim3(grid), dim3(QA_BLOCK),
        ldsBytes, stream, sv, nTiles, tb, colMax, piSign, (bitCapInt)0u, cplx<R>{ (R)0, (R)0 },
        tileSumsDev);
}

// k_qft_low_lds as a support-restricted pass (QftSupportArgs): the loop of
// k_qft_low_lds_var over the active tiles only, its source masked to the
// support. A sibling once more, so the kernels above compile as before.
template <typename R, int K, bool PRE, bool SUMS>
__global__ void __launch_bounds__(256, 3) k_qft_low_lds_sup(cplx<R>* sv, int tb, int colMax,
    R piSign, QftSupportArgs sup, cplx<R> phase, double* tileSums)
{
    // REQUIRES colMax+1 to be a multiple of K, as k_qft_low_lds does
    extern __shared__ unsigned char qa_lds_raw[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw);
    const int tile = 1 << tb;
    const int nCols = colMax + 1;
    const int nG = nCols / K;
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    const int firstG = PRE ? 0 : (nG - 1);
    const int lastG = PRE ? (nG - 1) : 0;
    const bool copyIn = (K * firstG) < 6;
    const bool copyOut = (K * lastG) < 6;
    for (bitCapInt c = blockIdx.x; c < sup.activeTiles; c += gridDim.x) {
        const bitCapInt t = qaSupportTile(c, sup.tileFree, sup.tileFixed);
        cplx<R>* svBase = sv + (t << tb);
        const bitCapInt idxBase = t << tb;
        double acc = 0;
        if (copyIn) {
            for (int j = threadIdx.x; j < tile; j += blockDim.x) {
                lds[qaSwz(j)] = qaSupportLoad<R>(svBase + j, idxBase | (bitCapInt)j, sup, phase);
            }
        }
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0) && !copyIn;
            const bool toGlobal = (gi == nG - 1) && !copyOut;
            const R scaleHi = piSign / (R)(1 << (gLo + K - 1));
            if (gi != 0 || copyIn) __syncthreads();
            qftLowGroup<R, K, PRE, false, SUMS, true>(svBase, lds, tile, gLo, scaleHi, iSign,
                fromGlobal, toGlobal, idxBase, 0u, phase, &acc, &sup);
        }
        if (copyOut) {
            __syncthreads();
            if (SUMS) {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) {
                    const cplx<R> a = lds[qaSwz(j)];
                    svBase[j] = a;
                    acc += (double)norm(a);
                }
            } else {
                for (int j = threadIdx.x; j < tile; j += blockDim.x) svBase[j] = lds[qaSwz(j)];
            }
        }
        if (SUMS) {
            // fixed-order block reduction, as in k_qft_low_lds_var
            __shared__ double waveSums[QA_BLOCK / 64];
            acc = waveReduceSum(acc);
            if ((threadIdx.x & 63) == 0) waveSums[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double s = 0;
                for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += waveSums[w];
                tileSums[t] = s;
            }
        }
        __syncthreads();
    }
}

// the active tiles of a support-restricted pass must lie inside the state
static void qaCheckSupportTiles(const QftSupportArgs& sup, bitCapInt nTiles)
{
    bitCapInt count = 1u;
    for (bitCapInt m = sup.tileFree; m; m &= m - 1u) count <<= 1u;
    if (!nTiles || (nTiles & (nTiles - 1u)) || ((sup.tileFree | sup.tileFixed) & ~(nTiles - 1u))
        || (sup.tileFree & sup.tileFixed) || sup.activeTiles != count) {
        throw QrackError("QFT support pass: tile subset outside the state");
    }
}

void launchQftLowLdsSupport(cplx<float>* sv, bitCapInt maxQPower, int tb, int colMax, int sign,
    bool pre, const QftSupportArgs& sup, cplx<float> phase, double* tileSumsDev,
    hipStream_t stream)
{
    constexpr int K = qaLowLadderK<float>();
    if (tb != qaLdsTileBits<float>() || (colMax + 1) % K || colMax >= tb) {
        throw QrackError("launchQftLowLdsSupport: ladder outside the tile or not K-aligned");
    }
    qaCheckSupportTiles(sup, maxQPower >> tb);
    if (pre && tileSumsDev) throw QrackError("launchQftLowLdsSupport: norms are forward-only");
    const size_t ldsBytes = (size_t(1) << tb) * sizeof(cplx<float>);
    const int grid = ldsGridFor(sup.activeTiles);
    const float piSign = (float)sign * 3.14159265358979323846f;
    if (pre) {
        hipLaunchKernelGGL((k_qft_low_lds_sup<float, K, true, false>), dim3(grid), dim3(QA_BLOCK),
            ldsBytes, stream, sv, tb, colMax, piSign, sup, phase, (double*)nullptr);
    } else if (tileSumsDev) {
        hipLaunchKernelGGL((k_qft_low_lds_sup<float, K, false, true>), dim3(grid), dim3(QA_BLOCK),
            ldsBytes, stream, sv, tb, colMax, piSign, sup, phase, tileSumsDev);
    } else {
        hipLaunchKernelGGL((k_qft_low_lds_sup<float, K, false, false>), dim3(grid),
            dim3(QA_BLOCK), ldsBytes, stream, sv, tb, colMax, piSign, sup, phase,
            (double*)nullptr);
    }
}

// ---- forward last low pass of a support plan: orbits with a nonzero only -----
//
// Entering this pass a tile holds one nonzero (12 columns) or sixteen (8
// columns), so in the first group one orbit in 256 has a nonzero input, in the
// next 16 in 256, and only the group at gLo = 0 all of them
// (qftSparseLastPlan). An orbit of sixteen +0 inputs is not dropped for +0
// outputs: its twiddles have signs, so it leaves signed zeros, and a later
// orbit with a nonzero input meets them (x·(+0) − y·(−0) and the like decide
// the sign of a zero component that is stored). Those zeros depend on the
// in-tile position alone. k_qft_sparse_zero_template runs the dense group
// code over a tile of +0 and keeps the two sign bits of every amplitude after
// each group but the last; k_qft_low_sparse_last runs the orbits with a
// nonzero input alone, takes their fifteen partners from that template, and
// so stores what k_qft_low_lds_sup stores, bit for bit. That rests on the
// compiler forming the same contracted arithmetic in both, which it does
// only for the same code shape: both kernels keep the dense loop and group
// body statement for statement (tests/test_qft_sparse_last_gpu.py and the
// byte comparisons of the support and lazy tests are the check).

constexpr int QA_SPARSE_THREADS = 256;

// per group in execution order: qftSparseLastPlan's below and slot
struct QftSparseLastArgs {
    int below[3];
    int slot[3];
};

// amplitude b of a template mask: bit 2b is the sign of re, bit 2b+1 of im
__device__ __forceinline__ cplx<float> qaSignedZero(uint32_t m, int b)
{
    return cplx<float>{ __uint_as_float((m << (31 - 2 * b)) & 0x80000000u),
        __uint_as_float((m << (30 - 2 * b)) & 0x80000000u) };
}

// tpl[g * 4096 + j], g = 0 / 1: sign bits (1: re, 2: im) of amplitude j, on
// entry to the group at gLo = 4 / gLo = 0 of an nG-group ladder, of a tile
// outside the support. The loop is k_qft_low_lds_sup's over one such tile
// (index 1 of a support that fixes every bit to 0: no input matches, none is
// loaded), without the last group and with the signs kept after each of the
// others. The group code must see its inputs arrive as in that kernel, from
// either source: the compiler contracts the orbit arithmetic differently
// when only one is left, and the zeros' signs follow the contraction.
// One block of QA_SPARSE_THREADS threads, one tile of LDS.
__global__ void __launch_bounds__(QA_SPARSE_THREADS)
    k_qft_sparse_zero_template(unsigned char* tpl, int nG, float piSign)
{
    extern __shared__ unsigned char qa_lds_raw[];
    cplx<float>* lds = reinterpret_cast<cplx<float>*>(qa_lds_raw);
    constexpr int K = 4;
    const int tb = 12;
    const int tile = 1 << tb;
    const float iSign = (piSign >= 0) ? 1.0f : -1.0f;
    const cplx<float> phase{ 0.0f, 0.0f };
    QftSupportArgs sup{};
    sup.fixedMask = ~(bitCapInt)0u;
    sup.fromBuffer = 1;
    const bitCapInt idxBase = (bitCapInt)1u << tb;
    cplx<float>* svBase = nullptr; // never dereferenced: no index is in the support
    const bool copyIn = (K * (nG - 1)) < 6;
    for (int j = threadIdx.x; j < tile; j += blockDim.x) {
        if (copyIn) {
            lds[qaSwz(j)] = qaSupportLoad<float>(svBase + j, idxBase | (bitCapInt)j, sup, phase);
        }
        tpl[j] = 0; // the inputs of the first group are +0 themselves
    }
    for (int gi = 0; gi + 1 < nG; ++gi) {
        const int gLo = K * (nG - 1 - gi);
        const bool fromGlobal = (gi == 0) && !copyIn;
        const float scaleHi = piSign / (float)(1 << (gLo + K - 1));
        if (gi != 0 || copyIn) __syncthreads();
        qftLowGroup<float, K, false, false, false, true>(svBase, lds, tile, gLo, scaleHi, iSign,
            fromGlobal, false, idxBase, 0u, phase, nullptr, &sup);
        __syncthreads();
        unsigned char* dst = tpl + (gi + 3 - nG) * tile;
        for (int j = threadIdx.x; j < tile; j += blockDim.x) {
            const cplx<float> a = lds[qaSwz(j)];
            dst[j] = (unsigned char)((__float_as_uint(a.re) >> 31)
                | ((__float_as_uint(a.im) >> 31) << 1));
        }
    }
}

// tiles a block of k_qft_low_sparse_last takes at a time, as a power of two
constexpr int QA_SPARSE_BATCH_LOG2 = 2;
constexpr int QA_SPARSE_BATCH = 1 << QA_SPARSE_BATCH_LOG2;
// amplitudes of a tile that the groups at gLo = 8 and gLo = 4 touch
constexpr int QA_SPARSE_COMPACT = 256;

// the low bits of a batch's tile counter through qaSupportTile's deposit:
// qaSupportTile(c0 | i) = qaSupportTile(c0) | qaSupportTileLow(i) for
// c0 a multiple of QA_SPARSE_BATCH and i below it
__device__ __forceinline__ bitCapInt qaSupportTileLow(int i, bitCapInt freeMask)
{
    bitCapInt t = 0u;
#pragma unroll
    for (int q = 0; q < QA_SPARSE_BATCH_LOG2; ++q) {
        if ((i >> q) & 1) t |= freeMask & (~freeMask + 1u);
        freeMask &= freeMask - 1u;
    }
    return t;
}

// an amplitude in LDS. cplx<float> is aligned to 4 bytes, which makes two
// 4-byte LDS accesses of it; every place of the images is aligned to 8.
__device__ __forceinline__ cplx<float> qaLdsGet(const cplx<float>* p)
{
    const float2 f = *reinterpret_cast<const float2*>(p);
    return cplx<float>{ f.x, f.y };
}
__device__ __forceinline__ void qaLdsPut(cplx<float>* p, cplx<float> a)
{
    *reinterpret_cast<float2*>(p) = make_float2(a.re, a.im);
}

// qftLowGroup's body (forward, MASKED) for one orbit with a nonzero input.
// The floating-point statements are qftLowGroup's, statement for statement
// and with both gather sources, so that the compiler forms the same
// arithmetic; only the indices differ. The orbit's sixteen places are
// img[qaSwz(r | (b << sh))]; a fromGlobal gather reads the tile at
// jr | (b << gLo). `below` is the orbit's index under gLo in the tile.
template <typename R, int K>
__device__ __forceinline__ void qftLowGroupReal(cplx<R>* svBase, cplx<R>* img, bool active, int r,
    int sh, int jr, int gLo, int below, R scaleHi, R iSign, bool fromGlobal, bitCapInt idxBase,
    cplx<R> phase, const QftSupportArgs* sup)
{
    constexpr int NS = 1 << K;
    if (active) {
        cplx<R> v[NS];
        if (fromGlobal) {
#pragma unroll
            for (int b = 0; b < NS; ++b) {
                const int j = jr | (b << gLo);
                v[b] = qaOpaque<R>(
                    qaSupportLoad<R>(svBase + j, idxBase | (bitCapInt)j, *sup, phase));
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) v[b] = qaLdsGet(img + qaSwz(r | (b << sh)));
        }
        R sn, cs;
        devSinCos<R>(scaleHi * (R)below, &sn, &cs);
        qftOrbitColumns<R, K, false>(v, iSign, cplx<R>{ cs, sn });
#pragma unroll
        for (int b = 0; b < NS; ++b) qaLdsPut(img + qaSwz(r | (b << sh)), v[b]);
    }
}

// |a|^2 as the dense kernels' write-out forms it, both products rounded and
// then added (there the compiler packs the two multiplications); left to
// contract, the compiler fuses one product into the addition here and the
// tile sums lose their last bits
__device__ __forceinline__ float qaNormUnfused(cplx<float> a)
{
#pragma clang fp contract(off)
    return a.re * a.re + a.im * a.im;
}

// one wave's LDS traffic in order: what its lanes stored before is what any
// of its lanes loads after
__device__ __forceinline__ void qaWaveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The forward last pass over the orbits with a nonzero input, T =
// QA_SPARSE_BATCH tiles at a time. A batch is T consecutive active tiles
// (qaSupportTile of c0 .. c0 + T - 1); the blocks stride over the batches.
//
// LDS: the 4096-amplitude tile image, then T compact images of 256.
// Between tiles the tile image holds the template: at index j the signed
// zero a tile outside the support holds there on entry to the group at
// gLo = 0. The groups at gLo = 8 and gLo = 4 touch only the 256 places
// with (j & 15) == perm & 15; those live in the tile's compact image at
// m = j >> 4, which between batches holds the signed zeros on entry to the
// group at gLo = 4.
//
// Stage A, for the whole batch: the T orbits of the group at gLo = 8 in T
// lanes of one wave (their T loads from HBM leave together; one orbit per
// wave occupies four SIMDs for the same latency and measured slower), a
// barrier, the 16 T orbits of the group at gLo = 4 in one wave, a barrier.
// An 8-column ladder has the copy-in of its 16 T in-support amplitudes
// instead of the first group. All steps share one inlined orbit body.
//
// Stage B, tile by tile with no block barrier: thread o moves its seed
// compact[o] to place 16 o + (perm & 15) of the tile image, gives the
// compact place back to its template, and runs orbit o of the group at
// gLo = 0 on places 16 o .. 16 o + 15. Wave w so owns [1024 w, 1024 w +
// 1024) and, after a wave-level fence, writes that out by itself,
// lane-contiguously, putting the template back behind itself. The waves
// drift apart: one's stores overlap another's arithmetic. (A 16-byte
// write-out and nontemporal stores were measured and gained nothing that
// stands clear of the noise: profiles/PROF_QFT_SPARSE_BATCH.md.)
//
// Tile sums: every wave keeps its partial of tile i in lane i and leaves it
// after the batch in a tile-image place that the next seed overwrites
// anyway; one barrier, then thread i adds the four in wave order. A
// tile's 4096 norms are fp32 values of nearly one exponent, their sum
// needs under 40 bits, so every order of summation gives the same double
// as the dense kernel's.
//
// Three block barriers per batch.
template <bool SUMS>
__global__ void __launch_bounds__(QA_SPARSE_THREADS, 4) k_qft_low_sparse_last(cplx<float>* sv,
    int tb, int colMax, float piSign, QftSupportArgs sup, QftSparseLastArgs sch, cplx<float> phase,
    const unsigned char* zeroTpl, double* tileSums)
{
    // REQUIRES tb = 12 and colMax + 1 = 8 or 12 (the launcher checks)
    constexpr int K = 4;
    constexpr int T = QA_SPARSE_BATCH;
    extern __shared__ unsigned char qa_lds_raw[];
    cplx<float>* lds = reinterpret_cast<cplx<float>*>(qa_lds_raw);
    const int tile = 1 << tb;
    cplx<float>* compact = lds + tile;
    const int nCols = colMax + 1;
    const int nG = nCols / K;
    const float iSign = (piSign >= 0) ? 1.0f : -1.0f;
    const bool copyIn = (K * (nG - 1)) < 6;
    const int below8 = sch.below[0];
    const int below4 = sch.below[nG - 2];
    int tid = (int)threadIdx.x;
    int lane = tid & 63;
    int wave = tid >> 6;
    // the template into LDS. mc keeps the signs of the sixteen places this
    // thread writes out, in write-out order (bit 2q: re, bit 2q+1: im)
    uint32_t mc = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int j = 1024 * wave + lane + 64 * q;
        const uint32_t bits = zeroTpl[tile + j] & 3u;
        mc |= bits << (2 * q);
        lds[qaSwz(j)] = qaSignedZero(bits, 0);
    }
    const uint32_t mseed = zeroTpl[(tid << 4) | below4] & 3u;
#pragma unroll
    for (int i = 0; i < T; ++i) compact[QA_SPARSE_COMPACT * i + qaSwz(tid)] = qaSignedZero(mseed, 0);
    __syncthreads();
    const bitCapInt nBatches = (sup.activeTiles + (bitCapInt)(T - 1)) >> QA_SPARSE_BATCH_LOG2;
    for (bitCapInt cb = blockIdx.x; cb < nBatches; cb += gridDim.x) {
        const bitCapInt c0 = cb << QA_SPARSE_BATCH_LOG2;
        const int nt = (sup.activeTiles - c0 < (bitCapInt)T) ? (int)(sup.activeTiles - c0) : T;
        const bitCapInt tHi = qaSupportTile(c0, sup.tileFree, sup.tileFixed);
        double keep = 0;
        // what follows from the thread index is formed again where it is
        // used: kept from ahead of the loops it costs the orbit registers
        asm volatile("" : "+v"(tid));
        if (copyIn) {
            const int i = tid >> 4;
            if (i < nt) {
                const bitCapInt t = tHi | qaSupportTileLow(i, sup.tileFree);
                const int j = ((tid & 15) << 8) | sch.below[0] | (sch.slot[0] << 4);
                compact[QA_SPARSE_COMPACT * i + qaSwz(j >> 4)] = qaSupportLoad<float>(
                    sv + (t << tb) + j, (t << tb) | (bitCapInt)j, sup, phase);
            }
        }
        // steps 0 and 1 are stage A, step 2 + i is tile i of stage B
        for (int st = copyIn ? 1 : 0; st < 2 + nt; ++st) {
            if (st == 1 || st == 2) __syncthreads();
            asm volatile("" : "+v"(tid));
            lane = tid & 63;
            wave = tid >> 6;
            // the wave of a stage A step changes from step to step, batch to
            // batch and block to block, so that they do not all queue on one
            // SIMD of the CU
            const int rot = 64 * (int)((cb + (cb >> 3) + (cb >> 8) + (bitCapInt)st) & 3u);
            const int x = (tid + rot) & (QA_SPARSE_THREADS - 1);
            int i, r, sh, gLo, below;
            if (st == 0) {
                i = x;
                r = below8 >> 4;
                sh = 4;
                gLo = 8;
                below = below8;
            } else if (st == 1) {
                i = x >> 4;
                r = (x & 15) << 4;
                sh = 0;
                gLo = 4;
                below = below4;
            } else {
                i = st - 2;
                r = tid << 4;
                sh = 0;
                gLo = 0;
                below = 0;
            }
            const bool stageB = st >= 2;
            const bitCapInt t = tHi | qaSupportTileLow(i, sup.tileFree);
            cplx<float>* svBase = sv + (t << tb);
            cplx<float>* cimg = compact + QA_SPARSE_COMPACT * i;
            if (stageB) {
                const int p = qaSwz(tid);
                lds[qaSwz(r | below4)] = cimg[p];
                cimg[p] = qaSignedZero(mseed, 0);
            }
            const float scaleHi = piSign / (float)(1 << (gLo + K - 1));
            qftLowGroupReal<float, K>(svBase, stageB ? lds : cimg, i < nt, r, sh, below8, gLo, below,
                scaleHi, iSign, st == 0, t << tb, phase, &sup);
            if (stageB) {
                qaWaveSync();
                // (i is uniform here) the write-out, with the signs taken from
                // mc place by place: formed ahead of the loop they would
                // cost 32 registers
                cplx<float>* svOut = sv + ((tHi | qaSupportTileLow(st - 2, sup.tileFree)) << tb);
                asm volatile("" : "+v"(mc));
                double acc = 0;
                int bit = 31;
                // amplitude k of the lane is j = 1024 wave + lane + 64 k. Bits
                // 6..9 of j are k and bits 4, 5 come from the lane, so
                // qaSwz(j) = (qaSwz(j0) ^ 4 (k & 3)) + 64 k: four bases and
                // constant offsets, in LDS and in the tile
                const int q0 = qaSwz(1024 * wave + lane);
                cplx<float>* outLane = svOut + (1024 * wave + lane);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    cplx<float>* place = lds + (q0 ^ ((k & 3) << 2)) + 64 * k;
                    const cplx<float> a = qaLdsGet(place);
                    outLane[64 * k] = a;
                    if (SUMS) acc += (double)qaNormUnfused(a);
                    qaLdsPut(place, cplx<float>{ __uint_as_float((mc << bit) & 0x80000000u),
                        __uint_as_float((mc << (bit - 1)) & 0x80000000u) });
                    bit -= 2;
                }
                qaWaveSync();
                if (SUMS) {
                    acc = waveReduceSum(acc);
                    const double tot = __shfl(acc, 0);
                    if (lane == i) keep = tot;
                }
            }
        }
        // the partials go where the seeds of the next batch land
        lane = tid & 63;
        wave = tid >> 6;
        if (SUMS && lane < nt) {
            *reinterpret_cast<double*>(lds + qaSwz(((64 * wave + lane) << 4) | below4)) = keep;
        }
        __syncthreads(); // the compact images are free again
        if (SUMS && tid < nt) {
            double s = 0;
            for (int w = 0; w < QA_SPARSE_THREADS / 64; ++w) {
                s += *reinterpret_cast<const double*>(lds + qaSwz(((64 * w + tid) << 4) | below4));
            }
            tileSums[tHi | qaSupportTileLow(tid, sup.tileFree)] = s;
        }
    }
}

static float qaForwardPiSign() { return (float)(+1) * 3.14159265358979323846f; }

void launchQftSparseZeroTemplate(unsigned char* zeroTplDev, int nCols, hipStream_t stream)
{
    if (!zeroTplDev || (nCols != 8 && nCols != 12)) {
        throw QrackError("launchQftSparseZeroTemplate: ladder of 8 or 12 columns only");
    }
    const size_t ldsBytes = (size_t(1) << 12) * sizeof(cplx<float>);
    hipLaunchKernelGGL(k_qft_sparse_zero_template, dim3(1), dim3(QA_SPARSE_THREADS), ldsBytes,
        stream, zeroTplDev, nCols / 4, qaForwardPiSign());
}

void launchQftLowSparseLast(cplx<float>* sv, bitCapInt maxQPower, int tb, int colMax,
    const QftSupportArgs& sup, cplx<float> phase, const unsigned char* zeroTplDev,
    double* tileSumsDev, hipStream_t stream)
{
    const int nCols = colMax + 1;
    const QftSparseLastPlan plan = qftSparseLastPlan(nCols, (unsigned long long)sup.perm);
    if (tb != 12 || tb != qaLdsTileBits<float>() || qaLowLadderK<float>() != 4 || !plan.eligible) {
        throw QrackError("launchQftLowSparseLast: ladder of 8 or 12 columns in a 4096-tile only");
    }
    qaCheckSupportTiles(sup, maxQPower >> tb);
    // the nonzeros of a tile must be where the schedule has them
    const bitCapInt tileMask = ((bitCapInt)1 << tb) - 1u;
    if ((sup.fixedMask & tileMask) != (((bitCapInt)1 << nCols) - 1u)) {
        throw QrackError("launchQftLowSparseLast: support does not match the ladder");
    }
    if (!zeroTplDev) throw QrackError("launchQftLowSparseLast: no zero template");
    QftSparseLastArgs sch{};
    for (size_t g = 0; g < plan.groups.size(); ++g) {
        sch.below[g] = plan.groups[g].below;
        sch.slot[g] = plan.groups[g].slot;
    }
    // the tile image and one compact image per tile of a batch; nothing
    // static beside them, so that four blocks share a CU's 160 KB
    const size_t ldsBytes = ((size_t(1) << tb) + (size_t)QA_SPARSE_BATCH * QA_SPARSE_COMPACT)
        * sizeof(cplx<float>);
    const int grid = ldsGridFor((sup.activeTiles + QA_SPARSE_BATCH - 1u) / QA_SPARSE_BATCH);
    const float piSign = qaForwardPiSign();
    if (tileSumsDev) {
        hipLaunchKernelGGL((k_qft_low_sparse_last<true>), dim3(grid), dim3(QA_SPARSE_THREADS),
            ldsBytes, stream, sv, tb, colMax, piSign, sup, sch, phase, zeroTplDev, tileSumsDev);
    } else {
        hipLaunchKernelGGL((k_qft_low_sparse_last<false>), dim3(grid), dim3(QA_SPARSE_THREADS),
            ldsBytes, stream, sv, tb, colMax, piSign, sup, sch, phase, zeroTplDev, tileSumsDev);
    }
}

// One group of K mid columns over a 64 x 2^nCols 2D tile as 16-amp register
// orbits (K templated — see qftLowGroup). Every access, LDS or HBM, keeps
// the 64-value `low` dimension in the lane index, so loads/stores are
// 512 B-contiguous per slot and LDS is bank-conflict-free without swizzle.
// BASIS: as in qftLowGroup — a fromGlobal gather is synthesised from the
// index of the basis state phase·|perm> instead of loaded.
// MASKED: as in qftLowGroup — the gather goes through qaSupportLoad.
template <typename R, int K, bool PRE, bool BASIS = false, bool MASKED = false>
__device__ __forceinline__ void qftMidGroup(cplx<R>* sv, cplx<R>* lds, bitCapInt xBase,
    int colLo, int tileAmps, int gLo, R midFixed, R hbScale, R scaleHi, R iSign,
    bool fromGlobal, bool toGlobal, bitCapInt perm = 0u, cplx<R> phase = cplx<R>{ (R)0, (R)0 },
    const QftSupportArgs* sup = nullptr)
{
    constexpr int NS = 1 << K;
    const int orbitCount = tileAmps >> K;
    for (int o = threadIdx.x; o < orbitCount; o += blockDim.x) {
        const int low = o & 63;
        const int cbr = o >> 6;
        const int cbBelow = cbr & ((1 << gLo) - 1);
        const int cb0 = ((cbr >> gLo) << (gLo + K)) | cbBelow;
        cplx<R> v[NS];
        if (fromGlobal) {
            if (MASKED) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    const bitCapInt x =
                        xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low;
                    v[b] = qaOpaque<R>(qaSupportLoad<R>(sv + x, x, *sup, phase));
                }
            } else if (BASIS) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    v[b] = qaOpaque<R>(
                        ((xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low) == perm)
                            ? phase
                            : cplx<R>{ (R)0, (R)0 });
                }
            } else {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    v[b] = sv[xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low];
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) v[b] = lds[((cb0 | (b << gLo)) << 6) | low];
        }
        R sn, cs;
        devSinCos<R>(scaleHi * ((R)low + midFixed + hbScale * (R)cbBelow), &sn, &cs);
        qftOrbitColumns<R, K, PRE>(v, iSign, cplx<R>{ cs, sn });
        if (toGlobal) {
#pragma unroll
            for (int b = 0; b < NS; ++b) {
                sv[xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low] = v[b];
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) lds[((cb0 | (b << gLo)) << 6) | low] = v[b];
        }
    }
}

// Up to SIX mid-range QFT columns per pass through a 2D LDS tile: 64
// contiguous low amplitudes (coalesced 512 B runs) x 2^nCols column-bit
// combinations. Column bits are processed in groups of (up to) 4 as
// 16-amplitude register orbits (qftOrbitColumns): the first group gathers
// straight from HBM, the last scatters straight back, LDS carries the tile
// between groups. Ramp for column col: theta = scale_col * (x mod 2^col)
// where x mod 2^col = low6 + midFixed + cbBelow*2^colLo — low6 varies
// in-tile, midFixed (bits 6..colLo-1) is tile-constant, cbBelow is the
// tile's below-group column bits. Requires a start-0 register, colLo >= 6.
template <typename R, int K, bool PRE>
__global__ void __launch_bounds__(256, 3)
    k_qft_mid_lds(cplx<R>* sv, bitCapInt nTiles, int colLo, int nCols, R piSign)
{
    // REQUIRES nCols to be a multiple of K (launcher picks K) so every
    // group is the single kernel-wide instantiation — no register spills.
    extern __shared__ unsigned char qa_lds_raw2[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw2);
    const int C = 1 << nCols;
    const int tileAmps = 64 * C;
    const int nG = nCols / K;
    const bitCapInt midMask = (ONE_BCI << (colLo - 6)) - 1u;
    const R hbScale = (R)(uint64_t)(ONE_BCI << colLo);
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const bitCapInt xBase =
            ((t >> (colLo - 6)) << (colLo + nCols)) | ((t & midMask) << 6);
        const R midFixed = (R)(uint64_t)((t & midMask) << 6);
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0);
            const bool toGlobal = (gi == nG - 1);
            const R scaleHi = piSign / (R)(ONE_BCI << (colLo + gLo + K - 1));
            if (gi != 0) __syncthreads();
            qftMidGroup<R, K, PRE>(sv, lds, xBase, colLo, tileAmps, gLo, midFixed, hbScale,
                scaleHi, iSign, fromGlobal, toGlobal);
        }
        __syncthreads();
    }
}

// k_qft_mid_lds as the first pass from the basis state phase·|perm> (see
// k_qft_low_lds_var): write-only, stores bit-identical to the normal kernel
template <typename R, int K, bool PRE>
__global__ void __launch_bounds__(256, 3) k_qft_mid_lds_basis(
    cplx<R>* sv, bitCapInt nTiles, int colLo, int nCols, R piSign, bitCapInt perm, cplx<R> phase)
{
    // REQUIRES nCols to be a multiple of K (launcher picks K) so every
    // group is the single kernel-wide instantiation — no register spills.
    extern __shared__ unsigned char qa_lds_raw2[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw2);
    const int C = 1 << nCols;
    const int tileAmps = 64 * C;
    const int nG = nCols / K;
    const bitCapInt midMask = (ONE_BCI << (colLo - 6)) - 1u;
    const R hbScale = (R)(uint64_t)(ONE_BCI << colLo);
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const bitCapInt xBase =
            ((t >> (colLo - 6)) << (colLo + nCols)) | ((t & midMask) << 6);
        const R midFixed = (R)(uint64_t)((t & midMask) << 6);
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0);
            const bool toGlobal = (gi == nG - 1);
            const R scaleHi = piSign / (R)(ONE_BCI << (colLo + gLo + K - 1));
            if (gi != 0) __syncthreads();
            qftMidGroup<R, K, PRE, true>(sv, lds, xBase, colLo, tileAmps, gLo, midFixed, hbScale,
                scaleHi, iSign, fromGlobal, toGlobal, perm, phase);
        }
        __syncthreads();
    }
}

template <typename R>
void launchQftMidLds(
    cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, int sign, bool pre, hipStream_t stream)
{
    const bitCapInt nTiles = maxQPower >> (6 + nCols);
    const size_t ldsBytes = (size_t(64) << nCols) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    const R piSign = (R)sign * (R)3.14159265358979323846;
    // uniform group width: 4 | nCols -> K=4, else 3 | nCols -> K=3 (the
    // engine only requests nCols in {4, 6}; other multiples also work)
    if ((nCols & 3) == 0) {
        if (pre) {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 4, true>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        } else {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 4, false>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        }
    } else if ((nCols % 3) == 0) {
        if (pre) {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 3, true>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        } else {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 3, false>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        }
    } else {
        if (pre) {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 2, true>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        } else {
            hipLaunchKernelGGL((k_qft_mid_lds<R, 2, false>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
                stream, sv, nTiles, colLo, nCols, piSign);
        }
    }
}

template <typename R, int K>
static void launchQftMidLdsBasisK(cplx<R>* sv, bitCapInt nTiles, int grid, size_t ldsBytes,
    int colLo, int nCols, R piSign, bool pre, bitCapInt perm, cplx<R> phase, hipStream_t stream)
{
    if (pre) {
        hipLaunchKernelGGL((k_qft_mid_lds_basis<R, K, true>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
            stream, sv, nTiles, colLo, nCols, piSign, perm, phase);
    } else {
        hipLaunchKernelGGL((k_qft_mid_lds_basis<R, K, false>), dim3(grid), dim3(QA_BLOCK),
            ldsBytes, stream, sv, nTiles, colLo, nCols, piSign, perm, phase);
    }
}

template <typename R>
void launchQftMidLdsBasis(cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, int sign,
    bool pre, bitCapInt perm, cplx<R> phase, hipStream_t stream)
{
    const bitCapInt nTiles = maxQPower >> (6 + nCols);
    const size_t ldsBytes = (size_t(64) << nCols) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    const R piSign = (R)sign * (R)3.14159265358979323846;
    // same group-width choice as launchQftMidLds
    if ((nCols & 3) == 0) {
        launchQftMidLdsBasisK<R, 4>(
            sv, nTiles, grid, ldsBytes, colLo, nCols, piSign, pre, perm, phase, stream);
    } else if ((nCols % 3) == 0) {
        launchQftMidLdsBasisK<R, 3>(
            sv, nTiles, grid, ldsBytes, colLo, nCols, piSign, pre, perm, phase, stream);
    } else {
        launchQftMidLdsBasisK<R, 2>(
            sv, nTiles, grid, ldsBytes, colLo, nCols, piSign, pre, perm, phase, stream);
    }
}

// Wide-tile mid pass: 2^LB contiguous low amplitudes x 2^nCols column-bit
// combinations, LB < 6, so a tile of the same LDS footprint carries more
// columns (LB = 4: 9 columns in 64 KB, 128-byte runs). A sibling of
// k_qft_mid_lds / qftMidGroup rather than a shared template: its LDS
// addressing differs (below) and the 64-wide kernels stay exactly as they
// compile today. Ramp arithmetic is the 64-wide kernel's with the split
// moved: `low` is the LB in-run bits, midFixed the tile-constant bits
// LB..colLo-1, cbBelow the tile's below-group column bits.
//
// LDS mapping: amplitude (cb, low) of the tile, cb = the nCols column bits,
// lives at element ((cb ^ ((cb >> K) & SW)) << LB) | low, SW = 2^(6-LB) - 1.
// A wave's 64 lanes cover 2^(6-LB) consecutive orbit rows cbr. In the
// gLo = 0 group those rows differ in cb bits K.. (cb = cbr << K | b), which
// unswizzled puts them a multiple of 2^(K+LB) elements apart, all on the
// same banks; XORing cb bits K.. into cb bits 0.. spreads them over
// 2^(6-LB) consecutive 2^LB-element rows, i.e. 64 distinct consecutive
// 8-byte elements per wave access. In the gLo >= K groups the rows already
// differ in cb bits 0.. and the XORed-in bits are group bits, the same for
// every lane of one access, so those stay conflict-free too. Bits K.. of cb
// are untouched, so the mapping is a bijection of the tile.
template <int K, int LB> __device__ __forceinline__ int qaWideRow(int cb)
{
    return (cb ^ ((cb >> K) & ((1 << (6 - LB)) - 1))) << LB;
}

// MASKED: as in qftLowGroup — the gather goes through qaSupportLoad.
template <typename R, int K, bool PRE, bool BASIS, int LB, int THREADS, bool MASKED = false>
__device__ __forceinline__ void qftMidGroupWide(cplx<R>* sv, cplx<R>* lds, bitCapInt xBase,
    int colLo, int tileAmps, int gLo, R midFixed, R hbScale, R scaleHi, R iSign,
    bool fromGlobal, bool toGlobal, bitCapInt perm, cplx<R> phase,
    const QftSupportArgs* sup = nullptr)
{
    constexpr int NS = 1 << K;
    const int orbitCount = tileAmps >> K;
    for (int o = threadIdx.x; o < orbitCount; o += THREADS) {
        const int low = o & ((1 << LB) - 1);
        const int cbr = o >> LB;
        const int cbBelow = cbr & ((1 << gLo) - 1);
        const int cb0 = ((cbr >> gLo) << (gLo + K)) | cbBelow;
        cplx<R> v[NS];
        if (fromGlobal) {
            if (MASKED) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    const bitCapInt x =
                        xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low;
                    v[b] = qaOpaque<R>(qaSupportLoad<R>(sv + x, x, *sup, phase));
                }
            } else if (BASIS) {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    v[b] = qaOpaque<R>(
                        ((xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low) == perm)
                            ? phase
                            : cplx<R>{ (R)0, (R)0 });
                }
            } else {
#pragma unroll
                for (int b = 0; b < NS; ++b) {
                    v[b] = sv[xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low];
                }
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) v[b] = lds[qaWideRow<K, LB>(cb0 | (b << gLo)) | low];
        }
        R sn, cs;
        devSinCos<R>(scaleHi * ((R)low + midFixed + hbScale * (R)cbBelow), &sn, &cs);
        qftOrbitColumns<R, K, PRE>(v, iSign, cplx<R>{ cs, sn });
        if (toGlobal) {
#pragma unroll
            for (int b = 0; b < NS; ++b) {
                sv[xBase | ((bitCapInt)(cb0 | (b << gLo)) << colLo) | (bitCapInt)low] = v[b];
            }
        } else {
#pragma unroll
            for (int b = 0; b < NS; ++b) lds[qaWideRow<K, LB>(cb0 | (b << gLo)) | low] = v[b];
        }
    }
}

// nCols = 9 (K = 3, three groups) or 8 (K = 4, two groups) mid columns per
// pass; THREADS threads per block, one 2^(LB+nCols)-amplitude tile at a
// time. BASIS: first pass from the basis state phase·|perm>, write-only,
// stores bit-identical to the normal instantiation (see k_qft_mid_lds_basis).
// Requires a start-0 register, colLo >= LB and nCols a multiple of K.
template <typename R, int K, bool PRE, bool BASIS, int LB, int THREADS>
__global__ void __launch_bounds__(THREADS) k_qft_mid_wide(
    cplx<R>* sv, bitCapInt nTiles, int colLo, int nCols, R piSign, bitCapInt perm, cplx<R> phase)
{
    extern __shared__ unsigned char qa_lds_raw3[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw3);
    const int tileAmps = (1 << LB) << nCols;
    const int nG = nCols / K;
    const bitCapInt midMask = (ONE_BCI << (colLo - LB)) - 1u;
    const R hbScale = (R)(uint64_t)(ONE_BCI << colLo);
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const bitCapInt xBase =
            ((t >> (colLo - LB)) << (colLo + nCols)) | ((t & midMask) << LB);
        const R midFixed = (R)(uint64_t)((t & midMask) << LB);
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0);
            const bool toGlobal = (gi == nG - 1);
            const R scaleHi = piSign / (R)(ONE_BCI << (colLo + gLo + K - 1));
            if (gi != 0) __syncthreads();
            qftMidGroupWide<R, K, PRE, BASIS, LB, THREADS>(sv, lds, xBase, colLo, tileAmps, gLo,
                midFixed, hbScale, scaleHi, iSign, fromGlobal, toGlobal, perm, phase);
        }
        __syncthreads();
    }
}

template <typename R, int K, bool PRE, bool BASIS, int LB, int THREADS>
static void launchQftMidWideOne(cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, R piSign,
    bitCapInt perm, cplx<R> phase, hipStream_t stream)
{
    const bitCapInt nTiles = maxQPower >> (LB + nCols);
    const size_t ldsBytes = (size_t(1) << (LB + nCols)) * sizeof(cplx<R>);
    const int grid = ldsGridFor(nTiles);
    auto kern = k_qft_mid_wide<R, K, PRE, BASIS, LB, THREADS>;
    if (ldsBytes >= 64u * 1024u) {
        // a tile at or above the default dynamic-LDS limit: raise it, once
        // per instantiation and device
        static std::mutex mtx;
        static std::vector<int> raised;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) throw QrackError("k_qft_mid_wide: no device");
        std::lock_guard<std::mutex> lock(mtx);
        if (std::find(raised.begin(), raised.end(), dev) == raised.end()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes) != hipSuccess) {
                throw QrackError("k_qft_mid_wide: cannot raise the dynamic LDS limit");
            }
            raised.push_back(dev);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), ldsBytes, stream, sv, nTiles, colLo, nCols,
        piSign, perm, phase);
}

template <typename R, bool BASIS, int LB>
static void launchQftMidWideLB(cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, R piSign,
    bool pre, bitCapInt perm, cplx<R> phase, hipStream_t stream)
{
    // 9 columns: K = 3, two orbits per thread; 8 columns: K = 4, one orbit
    // per thread of a block half the size
    constexpr int T9 = 32 << LB;
    constexpr int T8 = 16 << LB;
    if (nCols == 9) {
        if (pre) {
            launchQftMidWideOne<R, 3, true, BASIS, LB, T9>(
                sv, maxQPower, colLo, nCols, piSign, perm, phase, stream);
        } else {
            launchQftMidWideOne<R, 3, false, BASIS, LB, T9>(
                sv, maxQPower, colLo, nCols, piSign, perm, phase, stream);
        }
    } else if (nCols == 8) {
        if (pre) {
            launchQftMidWideOne<R, 4, true, BASIS, LB, T8>(
                sv, maxQPower, colLo, nCols, piSign, perm, phase, stream);
        } else {
            launchQftMidWideOne<R, 4, false, BASIS, LB, T8>(
                sv, maxQPower, colLo, nCols, piSign, perm, phase, stream);
        }
    } else {
        throw QrackError("launchQftMidWide: nCols must be 8 or 9");
    }
}

void launchQftMidWide(cplx<float>* sv, bitCapInt maxQPower, int lowBits, int colLo, int nCols,
    int sign, bool pre, bool basis, bitCapInt perm, cplx<float> phase, hipStream_t stream)
{
    if (colLo < lowBits || (maxQPower >> (colLo + nCols)) == 0u) {
        throw QrackError("launchQftMidWide: columns outside the state or below the run length");
    }
    const float piSign = (float)sign * 3.14159265358979323846f;
    if (lowBits == 4) {
        if (basis) {
            launchQftMidWideLB<float, true, 4>(
                sv, maxQPower, colLo, nCols, piSign, pre, perm, phase, stream);
        } else {
            launchQftMidWideLB<float, false, 4>(
                sv, maxQPower, colLo, nCols, piSign, pre, perm, phase, stream);
        }
    } else if (lowBits == 5) {
        if (basis) {
            launchQftMidWideLB<float, true, 5>(
                sv, maxQPower, colLo, nCols, piSign, pre, perm, phase, stream);
        } else {
            launchQftMidWideLB<float, false, 5>(
                sv, maxQPower, colLo, nCols, piSign, pre, perm, phase, stream);
        }
    } else {
        throw QrackError("launchQftMidWide: lowBits must be 4 or 5");
    }
}

// k_qft_mid_lds and k_qft_mid_wide as support-restricted passes
// (QftSupportArgs): the same loops over the active tiles only, the first
// group's source masked to the support. Siblings, so the kernels above
// compile as before.
template <typename R, int K, bool PRE>
__global__ void __launch_bounds__(256, 3) k_qft_mid_lds_sup(
    cplx<R>* sv, int colLo, int nCols, R piSign, QftSupportArgs sup, cplx<R> phase)
{
    // REQUIRES nCols to be a multiple of K, as k_qft_mid_lds does
    extern __shared__ unsigned char qa_lds_raw2[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw2);
    const int C = 1 << nCols;
    const int tileAmps = 64 * C;
    const int nG = nCols / K;
    const bitCapInt midMask = (ONE_BCI << (colLo - 6)) - 1u;
    const R hbScale = (R)(uint64_t)(ONE_BCI << colLo);
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    for (bitCapInt c = blockIdx.x; c < sup.activeTiles; c += gridDim.x) {
        const bitCapInt t = qaSupportTile(c, sup.tileFree, sup.tileFixed);
        const bitCapInt xBase =
            ((t >> (colLo - 6)) << (colLo + nCols)) | ((t & midMask) << 6);
        const R midFixed = (R)(uint64_t)((t & midMask) << 6);
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0);
            const bool toGlobal = (gi == nG - 1);
            const R scaleHi = piSign / (R)(ONE_BCI << (colLo + gLo + K - 1));
            if (gi != 0) __syncthreads();
            qftMidGroup<R, K, PRE, false, true>(sv, lds, xBase, colLo, tileAmps, gLo, midFixed,
                hbScale, scaleHi, iSign, fromGlobal, toGlobal, 0u, phase, &sup);
        }
        __syncthreads();
    }
}

template <typename R, int K, bool PRE, int LB, int THREADS>
__global__ void __launch_bounds__(THREADS) k_qft_mid_wide_sup(
    cplx<R>* sv, int colLo, int nCols, R piSign, QftSupportArgs sup, cplx<R> phase)
{
    extern __shared__ unsigned char qa_lds_raw3[];
    cplx<R>* lds = reinterpret_cast<cplx<R>*>(qa_lds_raw3);
    const int tileAmps = (1 << LB) << nCols;
    const int nG = nCols / K;
    const bitCapInt midMask = (ONE_BCI << (colLo - LB)) - 1u;
    const R hbScale = (R)(uint64_t)(ONE_BCI << colLo);
    const R iSign = (piSign >= 0) ? (R)1 : (R)-1;
    for (bitCapInt c = blockIdx.x; c < sup.activeTiles; c += gridDim.x) {
        const bitCapInt t = qaSupportTile(c, sup.tileFree, sup.tileFixed);
        const bitCapInt xBase =
            ((t >> (colLo - LB)) << (colLo + nCols)) | ((t & midMask) << LB);
        const R midFixed = (R)(uint64_t)((t & midMask) << LB);
        for (int gi = 0; gi < nG; ++gi) {
            const int g = PRE ? gi : (nG - 1 - gi);
            const int gLo = K * g;
            const bool fromGlobal = (gi == 0);
            const bool toGlobal = (gi == nG - 1);
            const R scaleHi = piSign / (R)(ONE_BCI << (colLo + gLo + K - 1));
            if (gi != 0) __syncthreads();
            qftMidGroupWide<R, K, PRE, false, LB, THREADS, true>(sv, lds, xBase, colLo, tileAmps,
                gLo, midFixed, hbScale, scaleHi, iSign, fromGlobal, toGlobal, 0u, phase, &sup);
        }
        __syncthreads();
    }
}

template <int K, bool PRE>
static void launchQftMidLdsSupportOne(cplx<float>* sv, int colLo, int nCols, float piSign,
    const QftSupportArgs& sup, cplx<float> phase, hipStream_t stream)
{
    const size_t ldsBytes = (size_t(64) << nCols) * sizeof(cplx<float>);
    const int grid = ldsGridFor(sup.activeTiles);
    hipLaunchKernelGGL((k_qft_mid_lds_sup<float, K, PRE>), dim3(grid), dim3(QA_BLOCK), ldsBytes,
        stream, sv, colLo, nCols, piSign, sup, phase);
}

template <int K, bool PRE, int LB, int THREADS>
static void launchQftMidWideSupportOne(cplx<float>* sv, int colLo, int nCols, float piSign,
    const QftSupportArgs& sup, cplx<float> phase, hipStream_t stream)
{
    const size_t ldsBytes = (size_t(1) << (LB + nCols)) * sizeof(cplx<float>);
    const int grid = ldsGridFor(sup.activeTiles);
    auto kern = k_qft_mid_wide_sup<float, K, PRE, LB, THREADS>;
    if (ldsBytes >= 64u * 1024u) {
        // raise the dynamic-LDS limit once per instantiation and device, as
        // launchQftMidWideOne does
        static std::mutex mtx;
        static std::vector<int> raised;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) throw QrackError("k_qft_mid_wide_sup: no device");
        std::lock_guard<std::mutex> lock(mtx);
        if (std::find(raised.begin(), raised.end(), dev) == raised.end()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes) != hipSuccess) {
                throw QrackError("k_qft_mid_wide_sup: cannot raise the dynamic LDS limit");
            }
            raised.push_back(dev);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), ldsBytes, stream, sv, colLo, nCols, piSign,
        sup, phase);
}

template <int LB>
static void launchQftMidWideSupportLB(cplx<float>* sv, int colLo, int nCols, float piSign,
    bool pre, const QftSupportArgs& sup, cplx<float> phase, hipStream_t stream)
{
    // block sizes of launchQftMidWideLB
    constexpr int T9 = 32 << LB;
    constexpr int T8 = 16 << LB;
    if (nCols == 9) {
        if (pre) {
            launchQftMidWideSupportOne<3, true, LB, T9>(sv, colLo, nCols, piSign, sup, phase, stream);
        } else {
            launchQftMidWideSupportOne<3, false, LB, T9>(sv, colLo, nCols, piSign, sup, phase, stream);
        }
    } else {
        if (pre) {
            launchQftMidWideSupportOne<4, true, LB, T8>(sv, colLo, nCols, piSign, sup, phase, stream);
        } else {
            launchQftMidWideSupportOne<4, false, LB, T8>(sv, colLo, nCols, piSign, sup, phase, stream);
        }
    }
}

void launchQftMidSupport(cplx<float>* sv, bitCapInt maxQPower, int lowBits, int colLo, int nCols,
    int sign, bool pre, const QftSupportArgs& sup, cplx<float> phase, hipStream_t stream)
{
    const bool wide = nCols >= 8;
    if (nCols < 2 || nCols > 9 || nCols == 7 || nCols == 5 || colLo < lowBits
        || (maxQPower >> (colLo + nCols)) == 0u || (wide ? (lowBits != 4 && lowBits != 5) : lowBits != 6)) {
        throw QrackError("launchQftMidSupport: columns or run length outside what the kernels take");
    }
    qaCheckSupportTiles(sup, maxQPower >> (lowBits + nCols));
    const float piSign = (float)sign * 3.14159265358979323846f;
    if (wide) {
        if (lowBits == 4) {
            launchQftMidWideSupportLB<4>(sv, colLo, nCols, piSign, pre, sup, phase, stream);
        } else {
            launchQftMidWideSupportLB<5>(sv, colLo, nCols, piSign, pre, sup, phase, stream);
        }
    } else if ((nCols & 3) == 0) {
        // same group-width choice as launchQftMidLds
        if (pre) launchQftMidLdsSupportOne<4, true>(sv, colLo, nCols, piSign, sup, phase, stream);
        else launchQftMidLdsSupportOne<4, false>(sv, colLo, nCols, piSign, sup, phase, stream);
    } else if ((nCols % 3) == 0) {
        if (pre) launchQftMidLdsSupportOne<3, true>(sv, colLo, nCols, piSign, sup, phase, stream);
        else launchQftMidLdsSupportOne<3, false>(sv, colLo, nCols, piSign, sup, phase, stream);
    } else {
        if (pre) launchQftMidLdsSupportOne<2, true>(sv, colLo, nCols, piSign, sup, phase, stream);
        else launchQftMidLdsSupportOne<2, false>(sv, colLo, nCols, piSign, sup, phase, stream);
    }
}

// GENERIC K-column fused QFT kernel (2^K-amplitude orbits). The per-column
// ramp factor for the slot with column-c's bit set is
//   f0^(2^(K-1-c)) · Π_{j<c} U(c-j)^(b_j),   U(d) = e^{i·sign·π/2^d}
// — one sincos (f0) plus K-1 constant roots of unity drive every ramp.
template <typename R, int K, bool PRE>
__global__ void k_qft_colK(cplx<R>* sv, bitCapInt orbits, const bitCapInt tPows0,
    const bitCapInt tPows1, const bitCapInt tPows2, const bitCapInt tPows3, const bitCapInt tPows4,
    bitLenInt rampStart, bitCapInt lowMask, R scaleHi)
{
    // tPows: [0]=lowest column bit ... [K-1]=highest
    const bitCapInt tP[5] = { tPows0, tPows1, tPows2, tPows3, tPows4 };
    const R s = (R)0.70710678118654752440;
    const R iSign = (scaleHi >= 0) ? (R)1 : (R)-1;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    // U(d) = e^{i·sign·π/2^d}, d = 1..K-1
    cplx<R> U[5];
    {
        R ang = iSign * (R)1.57079632679489661923; // π/2
        for (int d = 1; d < K; ++d) {
            R sn, cs;
            devSinCos<R>(ang, &sn, &cs);
            U[d] = cplx<R>{ cs, sn };
            ang = ang * (R)0.5;
        }
    }
    const int NS = 1 << K;
    for (bitCapInt k = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; k < orbits;
         k += stride) {
        bitCapInt r = k;
        for (int b = 0; b < K; ++b) r = insertZeroBitDev(r, tP[b]);
        bitCapInt idx[1 << K];
        for (int b = 0; b < NS; ++b) {
            bitCapInt x = r;
            for (int c = 0; c < K; ++c) {
                if (b & (1 << c)) x |= tP[c];
            }
            idx[b] = x;
        }
        cplx<R> v[1 << K];
        for (int b = 0; b < NS; ++b) v[b] = sv[idx[b]];
        const uint64_t lf = (uint64_t)((r >> rampStart) & lowMask);
        R sn, cs;
        devSinCos<R>(scaleHi * (R)lf, &sn, &cs);
        cplx<R> fPow[5]; // f0^(2^m): fPow[0]=f0, fPow[m]=fPow[m-1]^2
        fPow[0] = cplx<R>{ cs, sn };
        for (int m = 1; m < K; ++m) fPow[m] = fPow[m - 1] * fPow[m - 1];
        // slot bit c corresponds to column index (from hi): c=K-1 is hi
        auto column = [&](int c) {
            // H over axis bit c
            for (int b = 0; b < NS; ++b) {
                if (b & (1 << c)) continue;
                const int hb = b | (1 << c);
                const cplx<R> t = s * (v[b] + v[hb]);
                const cplx<R> u = s * (v[b] - v[hb]);
                v[b] = t;
                v[hb] = u;
            }
            // ramp on slots with bit c set
            for (int b = 0; b < NS; ++b) {
                if (!(b & (1 << c))) continue;
                cplx<R> f = fPow[K - 1 - c];
                for (int j = 0; j < c; ++j) {
                    if (b & (1 << j)) f = f * U[c - j];
                }
                v[b] = f * v[b];
            }
        };
        auto columnInv = [&](int c) {
            for (int b = 0; b < NS; ++b) {
                if (!(b & (1 << c))) continue;
                cplx<R> f = fPow[K - 1 - c];
                for (int j = 0; j < c; ++j) {
                    if (b & (1 << j)) f = f * U[c - j];
                }
                v[b] = f * v[b];
            }
            for (int b = 0; b < NS; ++b) {
                if (b & (1 << c)) continue;
                const int hb = b | (1 << c);
                const cplx<R> t = s * (v[b] + v[hb]);
                const cplx<R> u = s * (v[b] - v[hb]);
                v[b] = t;
                v[hb] = u;
            }
        };
        if (!PRE) {
            for (int c = K - 1; c >= 0; --c) column(c);
        } else {
            for (int c = 0; c < K; ++c) columnInv(c);
        }
        for (int b = 0; b < NS; ++b) sv[idx[b]] = v[b];
    }
}

template <typename R>
void launchQftColumnK(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    int kCols, const bitCapInt* tPows, int sign, bool pre, hipStream_t stream)
{
    // tPows[0..kCols-1] ascending (lowest column first); col = highest column
    const bitCapInt lowMask = (ONE_BCI << (col - (kCols - 1))) - 1u;
    const R scaleHi = (R)sign * (R)3.14159265358979323846 / (R)(ONE_BCI << col);
    const bitCapInt orbits = maxQPower >> kCols;
    if (kCols == 5) {
        if (pre) {
            hipLaunchKernelGGL((k_qft_colK<R, 5, true>), dim3(gridFor(orbits)), dim3(QA_BLOCK),
                0, stream, sv, orbits, tPows[0], tPows[1], tPows[2], tPows[3], tPows[4],
                rampStart, lowMask, scaleHi);
        } else {
            hipLaunchKernelGGL((k_qft_colK<R, 5, false>), dim3(gridFor(orbits)), dim3(QA_BLOCK),
                0, stream, sv, orbits, tPows[0], tPows[1], tPows[2], tPows[3], tPows[4],
                rampStart, lowMask, scaleHi);
        }
        return;
    }
    if (kCols != 4) return; // 2/3 have tuned float4 kernels
    if (pre) {
        hipLaunchKernelGGL((k_qft_colK<R, 4, true>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tPows[0], tPows[1], tPows[2], tPows[3], 0u, rampStart, lowMask,
            scaleHi);
    } else {
        hipLaunchKernelGGL((k_qft_colK<R, 4, false>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tPows[0], tPows[1], tPows[2], tPows[3], 0u, rampStart, lowMask,
            scaleHi);
    }
}

template <typename R>
void launchQftColumn3(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tHi, bitCapInt tMid, bitCapInt tLo, int sign, bool pre, hipStream_t stream)
{
    const bitCapInt lowMask = (ONE_BCI << (col - 2u)) - 1u;
    const R scaleHi = (R)sign * (R)3.14159265358979323846 / (R)(ONE_BCI << col);
    const bitCapInt orbits = maxQPower >> 3u;
    if constexpr (std::is_same_v<R, float>) {
        if (tLo >= 2u && (orbits & 1u) == 0u) {
            if (pre) {
                hipLaunchKernelGGL((k_qft_col3_v<true>), dim3(gridFor(orbits >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, orbits >> 1u, tHi, tMid, tLo, rampStart,
                    lowMask, (float)scaleHi);
            } else {
                hipLaunchKernelGGL((k_qft_col3_v<false>), dim3(gridFor(orbits >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, orbits >> 1u, tHi, tMid, tLo, rampStart,
                    lowMask, (float)scaleHi);
            }
            return;
        }
    }
    if (pre) {
        hipLaunchKernelGGL((k_qft_col3<R, true>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tHi, tMid, tLo, rampStart, lowMask, scaleHi);
    } else {
        hipLaunchKernelGGL((k_qft_col3<R, false>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tHi, tMid, tLo, rampStart, lowMask, scaleHi);
    }
}

template <typename R>
void launchQftColumn2(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tHi, bitCapInt tLo, int sign, bool pre, hipStream_t stream)
{
    // columns (col, col-1): ramp low-bit count = col-1 bits below tLo
    const bitCapInt lowMask = (ONE_BCI << (col - 1u)) - 1u;
    const R scaleHi = (R)sign * (R)3.14159265358979323846 / (R)(ONE_BCI << col);
    const bitCapInt orbits = maxQPower >> 2u;
    if constexpr (std::is_same_v<R, float>) {
        if (tLo >= 2u && (orbits & 1u) == 0u) {
            if (pre) {
                hipLaunchKernelGGL((k_qft_col2_v<true>), dim3(gridFor(orbits >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, orbits >> 1u, tHi, tLo, rampStart, lowMask,
                    (float)scaleHi);
            } else {
                hipLaunchKernelGGL((k_qft_col2_v<false>), dim3(gridFor(orbits >> 1u)),
                    dim3(QA_BLOCK), 0, stream, sv, orbits >> 1u, tHi, tLo, rampStart, lowMask,
                    (float)scaleHi);
            }
            return;
        }
    }
    if (pre) {
        hipLaunchKernelGGL((k_qft_col2<R, true>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tHi, tLo, rampStart, lowMask, scaleHi);
    } else {
        hipLaunchKernelGGL((k_qft_col2<R, false>), dim3(gridFor(orbits)), dim3(QA_BLOCK), 0,
            stream, sv, orbits, tHi, tLo, rampStart, lowMask, scaleHi);
    }
}

template <typename R>
void launchQftColumn(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tPow, int sign, bool pre, hipStream_t stream)
{
    const bitCapInt maxI = maxQPower >> 1u;
    const bitCapInt rampMask = (ONE_BCI << col) - 1u;
    const R scale = (R)sign * (R)3.14159265358979323846 / (R)(ONE_BCI << col);
    if constexpr (std::is_same_v<R, float>) {
        if (tPow >= 2u && (maxI & 1u) == 0u) {
            static const bool pipe = []() {
                if (const char* env = std::getenv("QRACK_GPU_QFT_PIPE")) return std::atoi(env) != 0;
                return false;
            }();
            if (pipe) {
                if (pre) {
                    hipLaunchKernelGGL((k_qft_col_v_pipe<true>), dim3(gridFor(maxI >> 1u)),
                        dim3(QA_BLOCK), 0, stream, sv, maxI, tPow, rampStart, rampMask, (float)scale);
                } else {
                    hipLaunchKernelGGL((k_qft_col_v_pipe<false>), dim3(gridFor(maxI >> 1u)),
                        dim3(QA_BLOCK), 0, stream, sv, maxI, tPow, rampStart, rampMask, (float)scale);
                }
                return;
            }
            if (pre) {
                hipLaunchKernelGGL((k_qft_col_v<true>), dim3(gridFor(maxI >> 1u)), dim3(QA_BLOCK),
                    0, stream, sv, maxI, tPow, rampStart, rampMask, (float)scale);
            } else {
                hipLaunchKernelGGL((k_qft_col_v<false>), dim3(gridFor(maxI >> 1u)), dim3(QA_BLOCK),
                    0, stream, sv, maxI, tPow, rampStart, rampMask, (float)scale);
            }
            return;
        }
    }
    if (pre) {
        hipLaunchKernelGGL((k_qft_col<R, true>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0, stream,
            sv, maxI, tPow, rampStart, rampMask, scale);
    } else {
        hipLaunchKernelGGL((k_qft_col<R, false>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0, stream,
            sv, maxI, tPow, rampStart, rampMask, scale);
    }
}

// ---- batched independent single-qubit gates ---------------------------------
// k distinct-target 2x2s in ONE pass: each lane owns a 2^k-amplitude orbit in
// registers (k <= 5 fp32 / 4 fp64), so k memory-bound passes collapse to one.

template <typename R, int K>
__global__ void __launch_bounds__(256, K >= 5 ? 2 : (K >= 3 ? 3 : 4))
    k_mtrx_batch(cplx<R>* sv, Batch1qArgs<R> a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < a.maxI; j += stride) {
        const bitCapInt base = expandBits(j, a.tPow, K);
        cplx<R> v[1 << K];
#pragma unroll
        for (int s = 0; s < (1 << K); ++s) {
            bitCapInt off = 0;
#pragma unroll
            for (int g = 0; g < K; ++g) {
                if (s & (1 << g)) off |= a.tPow[g];
            }
            v[s] = sv[base | off];
        }
#pragma unroll
        for (int g = 0; g < K; ++g) {
            const cplx<R> m0 = a.m[4 * g], m1 = a.m[4 * g + 1], m2 = a.m[4 * g + 2],
                          m3 = a.m[4 * g + 3];
#pragma unroll
            for (int s = 0; s < (1 << K); ++s) {
                if (s & (1 << g)) continue;
                const int t = s | (1 << g);
                const cplx<R> x = v[s], y = v[t];
                v[s] = m0 * x + m1 * y;
                v[t] = m2 * x + m3 * y;
            }
        }
#pragma unroll
        for (int s = 0; s < (1 << K); ++s) {
            bitCapInt off = 0;
#pragma unroll
            for (int g = 0; g < K; ++g) {
                if (s & (1 << g)) off |= a.tPow[g];
            }
            sv[base | off] = v[s];
        }
    }
}

// fp32 float4 variant (requires tPow[0] >= 2): each lane handles TWO adjacent
// orbits via 16 B loads/stores — full-line HBM streams like k_apply2x2_1v.
template <int K>
__global__ void __launch_bounds__(256, K >= 4 ? 2 : (K >= 3 ? 3 : 4))
    k_mtrx_batch_v(cplx<float>* sv, Batch1qArgs<float> a)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt half = a.maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt t = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; t < half; t += stride) {
        const bitCapInt base = expandBits(2u * t, a.tPow, K); // even: bit0 non-target
        float4 v[1 << K];
#pragma unroll
        for (int s = 0; s < (1 << K); ++s) {
            bitCapInt off = 0;
#pragma unroll
            for (int g = 0; g < K; ++g) {
                if (s & (1 << g)) off |= a.tPow[g];
            }
            v[s] = sv4[(base | off) >> 1u];
        }
#pragma unroll
        for (int g = 0; g < K; ++g) {
            const cplx<float> m0 = a.m[4 * g], m1 = a.m[4 * g + 1], m2 = a.m[4 * g + 2],
                              m3 = a.m[4 * g + 3];
#pragma unroll
            for (int s = 0; s < (1 << K); ++s) {
                if (s & (1 << g)) continue;
                const int tt = s | (1 << g);
                const cplx<float> x0{ v[s].x, v[s].y }, x1{ v[s].z, v[s].w };
                const cplx<float> y0{ v[tt].x, v[tt].y }, y1{ v[tt].z, v[tt].w };
                const cplx<float> a0 = m0 * x0 + m1 * y0, a1 = m0 * x1 + m1 * y1;
                const cplx<float> b0 = m2 * x0 + m3 * y0, b1 = m2 * x1 + m3 * y1;
                v[s] = make_float4(a0.re, a0.im, a1.re, a1.im);
                v[tt] = make_float4(b0.re, b0.im, b1.re, b1.im);
            }
        }
#pragma unroll
        for (int s = 0; s < (1 << K); ++s) {
            bitCapInt off = 0;
#pragma unroll
            for (int g = 0; g < K; ++g) {
                if (s & (1 << g)) off |= a.tPow[g];
            }
            sv4[(base | off) >> 1u] = v[s];
        }
    }
}

// ---- MFMA demonstration variant ---------------------------------------------
// The BASELINE north star calls for "MFMA used for the batched 2x2 complex
// mat-vec". A 2x2 complex gate on a pair (x, y) is the 4x4 REAL matrix
// G = [[m0.re,-m0.im,m1.re,-m1.im],[m0.im,m0.re,m1.im,m1.re],
//      [m2.re,-m2.im,m3.re,-m3.im],[m2.im,m2.re,m3.im,m3.re]] acting on
// (x.re, x.im, y.re, y.im). Each wave feeds v_mfma_f32_16x16x4_f32 with
// A[i][k] = G[i%4][k] (the gate replicated down the rows) and
// B[k][j] = component k of pair j, producing 16 pair results per MFMA.
// The workload is HBM-bound at ~0.1 flop/byte, so this is a correctness +
// counter demonstration (QRACK_GPU_MFMA=1), not the default path — the A/B
// numbers are recorded in profiles/KERNELS.md.
typedef float qa_f32x4 __attribute__((ext_vector_type(4)));

__global__ void k_apply2x2_1mfma(cplx<float>* sv, GateArgs<float> a)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned j16 = lane & 15u;   // B column / D column
    const unsigned kRow = lane >> 4u;  // A k-index / B k-index
    const bitCapInt p = a.qPowers[0];
    // gate as 4x4 real, row (lane&15)%4, column kRow
    const float G[4][4] = {
        { a.m[0].re, -a.m[0].im, a.m[1].re, -a.m[1].im },
        { a.m[0].im, a.m[0].re, a.m[1].im, a.m[1].re },
        { a.m[2].re, -a.m[2].im, a.m[3].re, -a.m[3].im },
        { a.m[2].im, a.m[2].re, a.m[3].im, a.m[3].re },
    };
    const float aVal = G[j16 & 3u][kRow];
    const bitCapInt wavesPerGrid = ((bitCapInt)gridDim.x * blockDim.x) >> 6u;
    const bitCapInt waveId = (((bitCapInt)blockIdx.x * blockDim.x + threadIdx.x) >> 6u);
    const bitCapInt nGroups = (a.maxI + 15u) >> 4u; // 16 pairs per wave step
    for (bitCapInt g = waveId; g < nGroups; g += wavesPerGrid) {
        const bitCapInt myPair = (g << 4u) | j16;
        float xre = 0, xim = 0, yre = 0, yim = 0;
        const bool live = myPair < a.maxI;
        bitCapInt i = 0;
        if (live) {
            i = ((myPair & ~(p - 1u)) << 1u) | (myPair & (p - 1u));
            const cplx<float> x = sv[i | a.offset1];
            const cplx<float> y = sv[i | a.offset2];
            xre = x.re;
            xim = x.im;
            yre = y.re;
            yim = y.im;
        }
        // B[k][j] = component k of pair j: pull from lane j via wave shuffle
        const int src = (int)j16;
        const float c0 = __shfl(xre, src, 64);
        const float c1 = __shfl(xim, src, 64);
        const float c2 = __shfl(yre, src, 64);
        const float c3 = __shfl(yim, src, 64);
        const float bVal = (kRow == 0u) ? c0 : (kRow == 1u) ? c1 : (kRow == 2u) ? c2 : c3;
        qa_f32x4 acc = { 0.f, 0.f, 0.f, 0.f };
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aVal, bVal, acc, 0, 0, 0);
        // D[row][col]: lane holds rows (lane>>4)*4 + t, col = lane&15; every
        // 16-lane group holds the full 4-vector of pair (lane&15) — group 0
        // writes back
        if (live && kRow == 0u) {
            sv[i | a.offset1] = cplx<float>{ acc[0], acc[1] };
            sv[i | a.offset2] = cplx<float>{ acc[2], acc[3] };
        }
    }
}

// ---- LDS-tiled low-bit gate batch -------------------------------------------
// Each workgroup stages a contiguous 2^QA_LDS_TILE_BITS-amplitude tile in
// LDS, applies every gate (targets all inside the tile) at LDS bandwidth,
// then writes the tile back: ONE global RMW pass for up to 12 fused gates,
// with bit-0 targets handled as cheaply as any other.

// Gates are applied in GROUPS of qaLdsBatchK<R>() (4 fp32 / 3 fp64) as
// 2^K-amplitude register orbits: one LDS read + butterfly chain in
// registers + one LDS write per amp per group, instead of a pair-RMW
// through LDS per GATE. The engine pads a.k to a multiple of K with
// identity gates on spare tile bits and sorts each group's targets
// ascending (1q gates on distinct targets commute, so order is free).
template <typename R> __global__ void k_mtrx_batch_lds(cplx<R>* sv, BatchLdsArgs<R> a)
{
    constexpr int TB = qaLdsTileBits<R>();
    constexpr int K = qaLdsBatchK<R>();
    constexpr int NS = 1 << K;
    __shared__ cplx<R> tile[1u << TB];
    constexpr unsigned TILE = 1u << TB;
    const bitCapInt nTiles = a.maxQPower >> TB;
    const int nG = a.k / K;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const bitCapInt base = t << TB;
        for (unsigned i = threadIdx.x; i < TILE; i += blockDim.x) {
            tile[qaSwz((int)i)] = sv[base + i];
        }
        __syncthreads();
        for (int gi = 0; gi < nG; ++gi) {
            const int g0 = gi * K;
            unsigned p[K];
#pragma unroll
            for (int g = 0; g < K; ++g) p[g] = (unsigned)a.tPow[g0 + g];
            for (unsigned o = threadIdx.x; o < (TILE >> K); o += blockDim.x) {
                unsigned r = o;
#pragma unroll
                for (int g = 0; g < K; ++g) r = ((r & ~(p[g] - 1u)) << 1u) | (r & (p[g] - 1u));
                cplx<R> v[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    unsigned off = r;
#pragma unroll
                    for (int g = 0; g < K; ++g) {
                        if (s & (1 << g)) off |= p[g];
                    }
                    v[s] = tile[qaSwz((int)off)];
                }
#pragma unroll
                for (int g = 0; g < K; ++g) {
                    const cplx<R> m0 = a.m[4 * (g0 + g)], m1 = a.m[4 * (g0 + g) + 1],
                                  m2 = a.m[4 * (g0 + g) + 2], m3 = a.m[4 * (g0 + g) + 3];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s & (1 << g)) continue;
                        const int hb = s | (1 << g);
                        const cplx<R> x = v[s], y = v[hb];
                        v[s] = m0 * x + m1 * y;
                        v[hb] = m2 * x + m3 * y;
                    }
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    unsigned off = r;
#pragma unroll
                    for (int g = 0; g < K; ++g) {
                        if (s & (1 << g)) off |= p[g];
                    }
                    tile[qaSwz((int)off)] = v[s];
                }
            }
            __syncthreads();
        }
        for (unsigned i = threadIdx.x; i < TILE; i += blockDim.x) {
            sv[base + i] = tile[qaSwz((int)i)];
        }
        __syncthreads();
    }
}

template <typename R>
void launchMtrx1qBatchLds(cplx<R>* sv, const BatchLdsArgs<R>& a, hipStream_t stream)
{
    const bitCapInt nTiles = a.maxQPower >> qaLdsTileBits<R>();
    const int grid = ldsGridFor(nTiles);
    hipLaunchKernelGGL((k_mtrx_batch_lds<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
}

// LDS-tiled two-qubit batch: each workgroup stages one tile, then applies
// every 4x4 (pair bits inside the tile) at LDS speed — one global RMW pass
// for a whole disjoint two-qubit layer segment.
template <typename R> __global__ void k_mtrx2q_batch_lds(cplx<R>* sv, Batch2qLdsArgs<R> a)
{
    constexpr int TB = qaLdsTileBits<R>();
    __shared__ cplx<R> tile[1u << TB];
    constexpr unsigned TILE = 1u << TB;
    const bitCapInt nTiles = a.maxQPower >> TB;
    for (bitCapInt t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const bitCapInt base = t << TB;
        for (unsigned i = threadIdx.x; i < TILE; i += blockDim.x) {
            tile[i] = sv[base + i];
        }
        __syncthreads();
        for (int g = 0; g < a.k; ++g) {
            const unsigned lo = (unsigned)a.p1[g];
            const unsigned hi = (unsigned)a.p2[g];
            const cplx<R>* m = &a.m[16 * g];
            for (unsigned j = threadIdx.x; j < (TILE >> 2); j += blockDim.x) {
                // expand j around lo then hi (lo < hi)
                unsigned i0 = ((j & ~(lo - 1u)) << 1u) | (j & (lo - 1u));
                i0 = ((i0 & ~(hi - 1u)) << 1u) | (i0 & (hi - 1u));
                const unsigned i1 = i0 | lo;
                const unsigned i2 = i0 | hi;
                const unsigned i3 = i0 | lo | hi;
                const cplx<R> v0 = tile[i0], v1 = tile[i1], v2 = tile[i2], v3 = tile[i3];
                tile[i0] = m[0] * v0 + m[1] * v1 + m[2] * v2 + m[3] * v3;
                tile[i1] = m[4] * v0 + m[5] * v1 + m[6] * v2 + m[7] * v3;
                tile[i2] = m[8] * v0 + m[9] * v1 + m[10] * v2 + m[11] * v3;
                tile[i3] = m[12] * v0 + m[13] * v1 + m[14] * v2 + m[15] * v3;
            }
            __syncthreads();
        }
        for (unsigned i = threadIdx.x; i < TILE; i += blockDim.x) {
            sv[base + i] = tile[i];
        }
        __syncthreads();
    }
}

template <typename R>
void launchMtrx2qBatchLds(cplx<R>* sv, const Batch2qLdsArgs<R>& a, hipStream_t stream)
{
    const bitCapInt nTiles = a.maxQPower >> qaLdsTileBits<R>();
    const int grid = ldsGridFor(nTiles);
    hipLaunchKernelGGL((k_mtrx2q_batch_lds<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
}

template <typename R> __global__ void k_mtrx_2q(cplx<R>* sv, Gate4x4Args<R> a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < a.maxI; j += stride) {
        bitCapInt i0 = ((j & ~(a.p1 - 1u)) << 1u) | (j & (a.p1 - 1u));
        i0 = ((i0 & ~(a.p2 - 1u)) << 1u) | (i0 & (a.p2 - 1u));
        const bitCapInt i1 = i0 | a.p1;
        const bitCapInt i2 = i0 | a.p2;
        const bitCapInt i3 = i0 | a.p1 | a.p2;
        const cplx<R> v0 = sv[i0], v1 = sv[i1], v2 = sv[i2], v3 = sv[i3];
        sv[i0] = a.m[0] * v0 + a.m[1] * v1 + a.m[2] * v2 + a.m[3] * v3;
        sv[i1] = a.m[4] * v0 + a.m[5] * v1 + a.m[6] * v2 + a.m[7] * v3;
        sv[i2] = a.m[8] * v0 + a.m[9] * v1 + a.m[10] * v2 + a.m[11] * v3;
        sv[i3] = a.m[12] * v0 + a.m[13] * v1 + a.m[14] * v2 + a.m[15] * v3;
    }
}

template <typename R>
void launchMtrx2q(cplx<R>* sv, const Gate4x4Args<R>& a, hipStream_t stream)
{
    hipLaunchKernelGGL((k_mtrx_2q<R>), dim3(gridFor(a.maxI)), dim3(QA_BLOCK), 0, stream, sv, a);
}

// ---- batched disjoint CNOTs: one permutation pass per layer ----------------

template <typename R> __global__ void k_cnot_batch(cplx<R>* sv, CnotBatchArgs a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < a.maxI; i += stride) {
        bitCapInt xm = 0;
        for (int j = 0; j < a.k; ++j) {
            if (i & a.cPow[j]) xm |= a.tPow[j];
        }
        const bitCapInt p = i ^ xm;
        if (p <= i) continue; // partner handles the swap (or xm == 0)
        const cplx<R> t = sv[i];
        sv[i] = sv[p];
        sv[p] = t;
    }
}

// fp32 float4 variant: adjacent amplitude pairs share xm when neither a
// control nor a target sits at bit 0
__global__ void k_cnot_batch_v(cplx<float>* sv, CnotBatchArgs a)
{
    float4* sv4 = reinterpret_cast<float4*>(sv);
    const bitCapInt half = a.maxI >> 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt q = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; q < half; q += stride) {
        const bitCapInt i = q << 1u;
        bitCapInt xm = 0;
        for (int j = 0; j < a.k; ++j) {
            if (i & a.cPow[j]) xm |= a.tPow[j];
        }
        const bitCapInt p = i ^ xm;
        if (p <= i) continue;
        const bitCapInt qi = i >> 1u, qp = p >> 1u;
        const float4 t = sv4[qi];
        sv4[qi] = sv4[qp];
        sv4[qp] = t;
    }
}

template <typename R> __global__ void k_cphase_pairs(cplx<R>* sv, CPhasePairsArgs a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < a.maxI; i += stride) {
        double th = 0;
        for (int j = 0; j < a.k; ++j) {
            if ((i & a.cPow[j]) && (i & a.tPow[j])) th += a.angle[j];
        }
        if (th == 0.0) continue;
        R s, c;
        devSinCos<R>((R)th, &s, &c);
        sv[i] = cplx<R>{ c, s } * sv[i];
    }
}

template <typename R>
void launchCPhasePairs(cplx<R>* sv, const CPhasePairsArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(
        (k_cphase_pairs<R>), dim3(gridFor(a.maxI)), dim3(QA_BLOCK), 0, stream, sv, a);
}

template <typename R>
void launchCnotBatch(cplx<R>* sv, const CnotBatchArgs& a, hipStream_t stream)
{
    if constexpr (std::is_same_v<R, float>) {
        bool low = false;
        for (int j = 0; j < a.k; ++j) {
            if (a.cPow[j] < 2u || a.tPow[j] < 2u) low = true;
        }
        if (!low && (a.maxI & 1u) == 0u) {
            hipLaunchKernelGGL((k_cnot_batch_v), dim3(gridFor(a.maxI >> 1u)), dim3(QA_BLOCK), 0,
                stream, sv, a);
            return;
        }
    }
    hipLaunchKernelGGL((k_cnot_batch<R>), dim3(gridFor(a.maxI)), dim3(QA_BLOCK), 0, stream, sv, a);
}

template <typename R>
void launchMtrx1qBatch(cplx<R>* sv, const Batch1qArgs<R>& a, hipStream_t stream)
{
    const int grid = gridFor(a.maxI);
    if constexpr (std::is_same_v<R, float>) {
        if (a.tPow[0] >= 2u && a.maxI >= 2u && (a.maxI & 1u) == 0u && a.k <= 4) {
            const int gridv = gridFor(a.maxI >> 1u);
            switch (a.k) {
            case 2:
                hipLaunchKernelGGL((k_mtrx_batch_v<2>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            case 3:
                hipLaunchKernelGGL((k_mtrx_batch_v<3>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            case 4:
                hipLaunchKernelGGL((k_mtrx_batch_v<4>), dim3(gridv), dim3(QA_BLOCK), 0, stream, sv, a);
                return;
            }
        }
    }
    switch (a.k) {
    case 2:
        hipLaunchKernelGGL((k_mtrx_batch<R, 2>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    case 3:
        hipLaunchKernelGGL((k_mtrx_batch<R, 3>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    case 4:
        hipLaunchKernelGGL((k_mtrx_batch<R, 4>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    case 5:
        hipLaunchKernelGGL((k_mtrx_batch<R, 5>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv, a);
        break;
    default:
        throw QrackError("launchMtrx1qBatch: k out of range");
    }
}

template <typename R> __global__ void k_phase_ramp_gen(cplx<R>* sv, bitCapInt maxI, RampArgs a)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt j = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; j < maxI; j += stride) {
        bitCapInt i = j;
        if (a.condPow) {
            i = (((j & ~(a.condPow - 1u)) << 1u) | (j & (a.condPow - 1u))) | a.condPow;
        }
        uint64_t frac = (uint64_t)((i >> a.rampStart) & a.inPlaceRelMask);
        for (int k = 0; k < a.nScattered; ++k) {
            if (i & a.sPow[k]) frac += a.sWeight[k];
        }
        const R theta = (R)a.scale * (R)frac;
        R s, c;
        devSinCos<R>(theta, &s, &c);
        sv[i] = cplx<R>{ c, s } * sv[i];
    }
}

template <typename R>
void launchPhaseRampGeneral(cplx<R>* sv, bitCapInt maxQPower, const RampArgs& a, hipStream_t stream)
{
    const bitCapInt maxI = a.condPow ? (maxQPower >> 1u) : maxQPower;
    hipLaunchKernelGGL(
        (k_phase_ramp_gen<R>), dim3(gridFor(maxI)), dim3(QA_BLOCK), 0, stream, sv, maxI, a);
}

// ---- sampling / inner product / marginals --------------------------------------

template <typename R>
__global__ void k_chunk_sums(const cplx<R>* sv, bitCapInt chunkLen, double* sums)
{
    // one block per contiguous chunk
    const bitCapInt lo = (bitCapInt)blockIdx.x * chunkLen;
    double s = 0;
    for (bitCapInt i = lo + threadIdx.x; i < lo + chunkLen; i += blockDim.x) {
        s += (double)norm(sv[i]);
    }
    s = waveReduceSum(s);
    __shared__ double waveSums[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) waveSums[wid] = s;
    __syncthreads();
    if (wid == 0) {
        double t = (lane < QA_BLOCK / 64) ? waveSums[lane] : 0.0;
        t = waveReduceSum(t);
        if (lane == 0) sums[blockIdx.x] = t;
    }
}

template <typename R>
void launchChunkSums(
    const cplx<R>* sv, bitCapInt nChunks, bitCapInt chunkLen, double* sumsDev, hipStream_t stream)
{
    hipLaunchKernelGGL(
        (k_chunk_sums<R>), dim3((uint32_t)nChunks), dim3(QA_BLOCK), 0, stream, sv, chunkLen, sumsDev);
}

// chunk sums from the per-tile sums a SUMS low-ladder pass left behind:
// one wave per chunk, each lane adds its strided share in index order, then
// the fixed wave shuffle tree — deterministic
__global__ void k_tile_chunk_sums(const double* tileSums, bitCapInt tilesPerChunk, double* sums)
{
    const double* src = tileSums + (bitCapInt)blockIdx.x * tilesPerChunk;
    double s = 0;
    for (bitCapInt j = threadIdx.x; j < tilesPerChunk; j += 64u) s += src[j];
    s = waveReduceSum(s);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

void launchTileChunkSums(const double* tileSumsDev, bitCapInt nChunks, bitCapInt tilesPerChunk,
    double* sumsDev, hipStream_t stream)
{
    hipLaunchKernelGGL(k_tile_chunk_sums, dim3((uint32_t)nChunks), dim3(64), 0, stream,
        tileSumsDev, tilesPerChunk, sumsDev);
}

// sv[perm] = amp (the one non-zero amplitude of a basis state)
template <typename R> __global__ void k_set_amp(cplx<R>* sv, bitCapInt perm, cplx<R> amp)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) sv[perm] = amp;
}

template <typename R>
void launchSetAmp(cplx<R>* sv, bitCapInt perm, cplx<R> amp, hipStream_t stream)
{
    hipLaunchKernelGGL((k_set_amp<R>), dim3(1), dim3(1), 0, stream, sv, perm, amp);
}

template <typename R>
__global__ void k_inner(
    const cplx<R>* a, const cplx<R>* b, bitCapInt maxI, double* partialsRe, double* partialsIm)
{
    double re = 0, im = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxI; i += stride) {
        const cplx<R> x = a[i];
        const cplx<R> y = b[i];
        // conj(b) * a
        re += (double)(y.re * x.re + y.im * x.im);
        im += (double)(y.re * x.im - y.im * x.re);
    }
    re = waveReduceSum(re);
    im = waveReduceSum(im);
    __shared__ double wr[QA_BLOCK / 64];
    __shared__ double wi2[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) {
        wr[wid] = re;
        wi2[wid] = im;
    }
    __syncthreads();
    if (wid == 0) {
        double tr = (lane < QA_BLOCK / 64) ? wr[lane] : 0.0;
        double ti = (lane < QA_BLOCK / 64) ? wi2[lane] : 0.0;
        tr = waveReduceSum(tr);
        ti = waveReduceSum(ti);
        if (lane == 0) {
            partialsRe[blockIdx.x] = tr;
            partialsIm[blockIdx.x] = ti;
        }
    }
}

template <typename R>
int launchInner(const cplx<R>* a, const cplx<R>* b, bitCapInt maxI, double* partialsRe,
    double* partialsIm, hipStream_t stream)
{
    const int grid = gridForReduce(maxI);
    hipLaunchKernelGGL(
        (k_inner<R>), dim3(grid), dim3(QA_BLOCK), 0, stream, a, b, maxI, partialsRe, partialsIm);
    return grid;
}

template <typename R, bool USE_LDS>
__global__ void k_part_probs(
    const cplx<R>* sv, bitCapInt maxQPower, bitLenInt start, bitLenInt length, double* probs)
{
    const bitCapInt lenMask = (ONE_BCI << length) - 1u;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    if constexpr (USE_LDS) {
        extern __shared__ __attribute__((aligned(16))) char smemRaw[];
        double* hist = reinterpret_cast<double*>(smemRaw);
        const bitCapInt nBins = ONE_BCI << length;
        for (bitCapInt p = threadIdx.x; p < nBins; p += blockDim.x) hist[p] = 0;
        __syncthreads();
        for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower;
             i += stride) {
            const bitCapInt p = (i >> start) & lenMask;
            atomicAdd(&hist[p], (double)norm(sv[i]));
        }
        __syncthreads();
        for (bitCapInt p = threadIdx.x; p < nBins; p += blockDim.x) {
            if (hist[p] != 0.0) atomicAdd(&probs[p], hist[p]);
        }
    } else {
        for (bitCapInt i = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; i < maxQPower;
             i += stride) {
            const bitCapInt p = (i >> start) & lenMask;
            atomicAdd(&probs[p], (double)norm(sv[i]));
        }
    }
}

template <typename R>
void launchPartProbs(const cplx<R>* sv, bitCapInt maxQPower, bitLenInt start, bitLenInt length,
    double* probsDev, hipStream_t stream)
{
    const int grid = gridFor(maxQPower);
    const bitCapInt nBins = ONE_BCI << length;
    if (nBins <= 2048u) {
        hipLaunchKernelGGL((k_part_probs<R, true>), dim3(grid), dim3(QA_BLOCK),
            (uint32_t)(nBins * sizeof(double)), stream, sv, maxQPower, start, length, probsDev);
    } else {
        hipLaunchKernelGGL((k_part_probs<R, false>), dim3(grid), dim3(QA_BLOCK), 0, stream, sv,
            maxQPower, start, length, probsDev);
    }
}

// ---- Pauli pair walk --------------------------------------------------------------
//
// P|i> = i^ny (-1)^popcount(i&z) |i^x>. Every kernel from here to
// k_krylov_finish walks the index pairs (i, j = i^x) of one group of terms that
// share x, and only the half-space with the top bit of x clear: every amplitude
// of every vector involved is loaded once and, where written, stored once by
// exactly one thread. PairItem states the addressing; the kernels below are
// arithmetic over its lanes.
//
// An item is one 16-byte access per stream: one amplitude in fp64, two in fp32.
//   MODE 0  fp64: one pair per item, a = psi[i], b = psi[i^x].
//   MODE 1  fp32, x != 1: two pairs per item. i is even and i + 1 shares the
//           float4; the partner vector sits at i ^ (x & ~1), and with bit 0 of
//           x set its halves are swapped in registers on load and swapped back
//           before a store.
//   MODE 2  fp32, x == 1: the pair is the two halves of one vector.
//   MODE -1 x == 0 (the diagonal kernels): no partner, only the a lanes; two
//           in fp32, one in fp64.
// Lane l of a holds index i + l, lane l of b its partner (i + l) ^ x.
template <typename R, int MODE> struct PairItem {
    static constexpr bool F32 = sizeof(R) == 4;
    static_assert(MODE == -1 || (MODE == 0) == !F32, "MODE 0 is fp64, MODE 1 and 2 are fp32");
    static constexpr int L = (MODE == 1 || (MODE == -1 && F32)) ? 2 : 1;
    static constexpr bool TWO = (L == 2);
    using Vec = std::conditional_t<F32, float4, double2>;

    bitCapInt i;      // amplitude index of lane 0 of a
    bitCapInt ia, ib; // vector index of the a lanes and of the b lanes
    bool swapped;     // the b vector holds lane 1 in its lower half

    __device__ __forceinline__ PairItem(bitCapInt v, bitCapInt topPow, bitCapInt x)
    {
        if constexpr (MODE == 0) {
            i = ((v & ~(topPow - 1u)) << 1u) | (v & (topPow - 1u));
            ia = i;
            ib = i ^ x;
        } else if constexpr (MODE == 1) {
            const bitCapInt j = v << 1u;
            i = ((j & ~(topPow - 1u)) << 1u) | (j & (topPow - 1u));
            ia = i >> 1u;
            ib = (i ^ x) >> 1u;
        } else {
            i = F32 ? (v << 1u) : v;
            ia = ib = v;
        }
        swapped = (MODE == 1) && (x & 1u) != 0;
    }

    // NT (nontemporal access) exists for the float4 streams only
    template <bool NT> static __device__ __forceinline__ Vec ldv(const cplx<R>* p, bitCapInt k)
    {
        if constexpr (F32) return ld4<NT>(reinterpret_cast<const float4*>(p) + k);
        else return reinterpret_cast<const double2*>(p)[k];
    }
    template <bool NT> static __device__ __forceinline__ void stv(cplx<R>* p, bitCapInt k, Vec V)
    {
        if constexpr (F32) st4<NT>(reinterpret_cast<float4*>(p) + k, V);
        else reinterpret_cast<double2*>(p)[k] = V;
    }
    // one vector <-> its lower amplitude and, in fp32, its upper one
    static __device__ __forceinline__ void unpack(Vec V, cplx<R>& lo, cplx<R>& hi)
    {
        lo = cplx<R>(V.x, V.y);
        if constexpr (F32) hi = cplx<R>(V.z, V.w);
    }
    static __device__ __forceinline__ Vec pack(cplx<R> lo, cplx<R> hi)
    {
        if constexpr (F32) return make_float4(lo.re, lo.im, hi.re, hi.im);
        else return make_double2(lo.re, lo.im);
    }

    // the a lanes alone (MODE -1)
    template <bool NT = false> __device__ __forceinline__ void load(const cplx<R>* p, cplx<R> (&a)[L]) const
    {
        static_assert(MODE != 2, "in MODE 2 the vector's upper half is b");
        unpack(ldv<NT>(p, ia), a[0], a[L - 1]);
    }
    template <bool NT = false> __device__ __forceinline__ void store(cplx<R>* p, const cplx<R> (&a)[L]) const
    {
        stv<NT>(p, ia, pack(a[0], a[L - 1]));
    }

    template <bool NT = false>
    __device__ __forceinline__ void load(const cplx<R>* p, cplx<R> (&a)[L], cplx<R> (&b)[L]) const
    {
        if constexpr (MODE == 2) {
            unpack(ldv<NT>(p, ia), a[0], b[0]);
        } else {
            load<NT>(p, a);
            Vec B = ldv<NT>(p, ib);
            if constexpr (TWO) B = swapped ? make_float4(B.z, B.w, B.x, B.y) : B;
            unpack(B, b[0], b[L - 1]);
        }
    }
    template <bool NT = false>
    __device__ __forceinline__ void store(cplx<R>* p, const cplx<R> (&a)[L], const cplx<R> (&b)[L]) const
    {
        if constexpr (MODE == 2) {
            stv<NT>(p, ia, pack(a[0], b[0]));
        } else {
            Vec B = pack(b[0], b[L - 1]);
            if constexpr (TWO) B = swapped ? make_float4(B.z, B.w, B.x, B.y) : B;
            store<NT>(p, a);
            stv<NT>(p, ib, B);
        }
    }
};

// f(l) for every lane l < L, l a compile-time constant. A `#pragma unroll`
// loop over the lanes computes the same, but the lane arrays then reach
// registers only after the unroller has run, and the fp32 kernels come out
// with up to ten more VGPRs (profiles/PROF_PAIR_WALK.md).
template <int L, typename F> __device__ __forceinline__ void forLanes(F&& f)
{
    f(std::integral_constant<int, 0>{});
    if constexpr (L == 2) f(std::integral_constant<int, 1>{});
}

template <int MODE> using PairMode = std::integral_constant<int, MODE>;

// The mode of (x, nAmps) as a compile-time constant:
// f(PairMode<MODE>{}, nItems, topPow), topPow the top bit of x.
template <typename R, typename F> static void pauliPairDispatch(bitCapInt x, bitCapInt nAmps, F&& f)
{
    constexpr bool F32 = sizeof(R) == 4;
    if (!x) {
        f(PairMode<-1>{}, F32 ? (nAmps >> 1u) : nAmps, (bitCapInt)0);
        return;
    }
    const bitCapInt topPow = ONE_BCI << (63 - __builtin_clzll(x));
    if constexpr (!F32) {
        f(PairMode<0>{}, nAmps >> 1u, topPow);
    } else if (x == 1u) {
        f(PairMode<2>{}, nAmps >> 1u, topPow);
    } else {
        f(PairMode<1>{}, nAmps >> 2u, topPow);
    }
}

// a runtime flag as a template argument: f(std::true_type{}) or
// f(std::false_type{}); with CAN false the true form is never instantiated
template <bool CAN = true, typename F> static void liftBool(bool flag, F&& f)
{
    if constexpr (CAN) {
        if (flag) {
            f(std::true_type{});
            return;
        }
    }
    f(std::false_type{});
}

// grid of the pair kernels: one partial per block, and the QRACK_GPU_BLOCKS
// cap so that a small state can drive the stride loop
static inline int gridForPairs(bitCapInt nItems)
{
    int grid = gridForReduce(nItems);
    const int cap = maxBlocks();
    if (cap > 0 && grid > cap) grid = cap;
    return grid;
}

// block sum in a fixed order: wave shuffle -> LDS -> one double
__device__ __forceinline__ void blockSumStore(double s, double* dst)
{
    s = waveReduceSum(s);
    __shared__ double waveSums[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) waveSums[wid] = s;
    __syncthreads();
    if (wid == 0) {
        double t = (lane < QA_BLOCK / 64) ? waveSums[lane] : 0.0;
        t = waveReduceSum(t);
        if (lane == 0) *dst = t;
    }
}

// block sums of a complex value in a fixed order; the two parts have an LDS
// array each (two calls of blockSumStore would race on its one array)
__device__ __forceinline__ void blockSumStore2(double re, double im, double* dstRe, double* dstIm)
{
    re = waveReduceSum(re);
    im = waveReduceSum(im);
    __shared__ double waveRe[QA_BLOCK / 64];
    __shared__ double waveIm[QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) {
        waveRe[wid] = re;
        waveIm[wid] = im;
    }
    __syncthreads();
    if (wid == 0) {
        double tr = (lane < QA_BLOCK / 64) ? waveRe[lane] : 0.0;
        double ti = (lane < QA_BLOCK / 64) ? waveIm[lane] : 0.0;
        tr = waveReduceSum(tr);
        ti = waveReduceSum(ti);
        if (lane == 0) {
            *dstRe = tr;
            *dstIm = ti;
        }
    }
}

// stage 2: fold one launch's block partials, in a fixed order, into one double
__global__ void k_pauli_finish(const double* partials, int n, double* result)
{
    double s = 0;
    for (int k = threadIdx.x; k < n; k += QA_BLOCK) s += partials[k];
    blockSumStore(s, result);
}

// ... of a complex value, into (re, im)
__global__ void k_pauli_finish2(const double* partialsRe, const double* partialsIm, int n, double* result)
{
    double re = 0, im = 0;
    for (int k = threadIdx.x; k < n; k += QA_BLOCK) {
        re += partialsRe[k];
        im += partialsIm[k];
    }
    blockSumStore2(re, im, result, result + 1);
}

// w[l] = sum_t c_t (-1)^popcount((i + l) & z_t) over terms first .. last - 1;
// i is even when L == 2
template <int L, typename ARGS>
__device__ __forceinline__ void pauliWeights(const ARGS& a, int first, int last, bitCapInt i, double (&w)[L])
{
    w[0] = 0;
    w[L - 1] = 0;
    for (int t = first; t < last; ++t) {
        const bitCapInt z = a.z[t];
        const double c = a.w[t];
        const unsigned p0 = __popcll(i & z) & 1u;
        w[0] += p0 ? -c : c;
        if constexpr (L == 2) {
            const unsigned p1 = p0 ^ (unsigned)(z & 1u);
            w[1] += p1 ? -c : c;
        }
    }
}

// sum of |a[l]|^2 over the lanes, and of w[l] |a[l]|^2: squares in R, the rest
// in double
template <typename R, int L> __device__ __forceinline__ double pauliLaneNorm(const cplx<R> (&a)[L])
{
    if constexpr (L == 2) return (double)norm(a[0]) + (double)norm(a[1]);
    else return (double)norm(a[0]);
}
template <typename R, int L>
__device__ __forceinline__ double pauliLaneWeightedNorm(const double (&w)[L], const cplx<R> (&a)[L])
{
    if constexpr (L == 2) return w[0] * (double)norm(a[0]) + w[1] * (double)norm(a[1]);
    else return w[0] * (double)norm(a[0]);
}

// ---- Pauli-sum expectation -------------------------------------------------------
//
// <psi|P|psi>: for x != 0 the pair (i, i^x) contributes
// 2 Re(w(i) conj(psi[i^x]) psi[i]) with w(i) = sum_t c_t i^ny_t (-1)^popcount(i&z_t).
// Nothing is stored.

// 2 Re((wr + i wi) conj(b) a)
template <typename R> __device__ __forceinline__ double pauliPair(cplx<R> a, cplx<R> b, double wr, double wi)
{
    const R pr = b.re * a.re + b.im * a.im;
    const R pi = b.re * a.im - b.im * a.re;
    return 2.0 * (wr * (double)pr - wi * (double)pi);
}

template <typename R, int MODE>
__global__ void k_pauli_group(const cplx<R>* sv, PauliArgs a, bitCapInt nItems, bitCapInt topPow,
    double* partials)
{
    using Item = PairItem<R, MODE>;
    constexpr int L = Item::L;
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, topPow, a.x);
        cplx<R> A[L], B[L];
        double wr[L], wi[L];
        it.load(sv, A, B);
        pauliWeights(a, 0, a.nRe, it.i, wr);
        pauliWeights(a, a.nRe, a.nTerms, it.i, wi);
        forLanes<L>([&](auto l) { s += pauliPair(A[l], B[l], wr[l], wi[l]); });
    }
    blockSumStore(s, partials + blockIdx.x);
}

// x == 0: sum_i |psi[i]|^2 sum_t c_t (-1)^popcount(i&z_t)
template <typename R> __global__ void k_pauli_diag(const cplx<R>* sv, PauliArgs a, bitCapInt nItems, double* partials)
{
    using Item = PairItem<R, -1>;
    constexpr int L = Item::L;
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, 0u, 0u);
        cplx<R> A[L];
        double w[L];
        it.load(sv, A);
        pauliWeights(a, 0, a.nTerms, it.i, w);
        s += pauliLaneWeightedNorm(w, A);
    }
    blockSumStore(s, partials + blockIdx.x);
}

template <typename R>
void launchPauliGroup(const cplx<R>* sv, const PauliArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream)
{
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        constexpr int MODE = decltype(mode)::value;
        const int grid = gridForPairs(nItems);
        const dim3 g(grid), b(QA_BLOCK);
        if constexpr (MODE < 0) {
            hipLaunchKernelGGL((k_pauli_diag<R>), g, b, 0, stream, sv, a, nItems, partialsDev);
        } else {
            hipLaunchKernelGGL((k_pauli_group<R, MODE>), g, b, 0, stream, sv, a, nItems, topPow, partialsDev);
        }
        hipLaunchKernelGGL(k_pauli_finish, dim3(1), b, 0, stream, partialsDev, grid, resultDev);
    });
}

// ---- Pauli-sum evolution ---------------------------------------------------------
//
// exp(-i tau sum_t w_t P_t) for terms that share x, applied in place: the
// per-pair algebra is in qengine.hpp (pauliEvolvePlan).

// c[l] + i s[l] = e^{i angle} for segment k (its terms start at `first`) at
// index i + l. SINGLE: the segment is one term, |angle| is constant and the
// host's cos / sin are used, so only sin's sign depends on the index. Otherwise
// the angle is summed in double and sincos is the accurate double one: the
// native fast sincos is off by ~10 eps (ARCHITECTURE.md, cphase_pairs).
template <bool SINGLE, int L, typename R>
__device__ __forceinline__ void pauliEvolveCS(const PauliEvolveArgs& a, int k, int first, bitCapInt i,
    R (&c)[L], R (&s)[L])
{
    if constexpr (SINGLE) {
        const bitCapInt z = a.z[first];
        const unsigned p0 = __popcll(i & z) & 1u;
        const R cs = (R)a.segCos[k];
        const R sn = (R)a.segSin[k];
        c[0] = cs;
        s[0] = p0 ? -sn : sn;
        if constexpr (L == 2) {
            c[1] = cs;
            s[1] = (p0 ^ (unsigned)(z & 1u)) ? -sn : sn;
        }
    } else {
        double w[L], sd, cd;
        pauliWeights(a, first, a.segEnd[k], i, w);
        forLanes<L>([&](auto l) {
            sincos(w[l], &sd, &cd);
            c[l] = (R)cd;
            s[l] = (R)sd;
        });
    }
}

// re set: (a, b) <- (c a - i s b, c b - i s a); im set: (a, b) <- (c a - s b, c b + s a)
template <typename R> __device__ __forceinline__ void pauliEvolveRot(bool im, R c, R s, cplx<R>& a, cplx<R>& b)
{
    const R par = a.re, pai = a.im, pbr = b.re, pbi = b.im;
    if (im) {
        a.re = c * par - s * pbr;
        a.im = c * pai - s * pbi;
        b.re = c * pbr + s * par;
        b.im = c * pbi + s * pai;
    } else {
        a.re = c * par + s * pbi;
        a.im = c * pai - s * pbr;
        b.re = c * pbr + s * pai;
        b.im = c * pbi - s * par;
    }
}

// a <- (pr + i pi) a
template <typename R> __device__ __forceinline__ void pauliEvolveScale(R pr, R pi, cplx<R>& a)
{
    const R t = pr * a.re - pi * a.im;
    a.im = pr * a.im + pi * a.re;
    a.re = t;
}

template <typename R, int MODE, bool SINGLE, bool NT>
__global__ void k_pauli_evolve(cplx<R>* sv, PauliEvolveArgs a, bitCapInt nItems, bitCapInt topPow)
{
    using Item = PairItem<R, MODE>;
    constexpr int L = Item::L;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const R pr = (R)a.phaseRe, pi = (R)a.phaseIm;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, topPow, a.x);
        cplx<R> A[L], B[L];
        it.template load<NT>(sv, A, B);
        // Two lanes go round the segment loop as their two float4: carried as
        // eight scalars they cost up to ten more VGPRs and a wave of occupancy
        // (profiles/PROF_PAIR_WALK.md).
        [[maybe_unused]] typename Item::Vec VA, VB;
        if constexpr (L == 2) VA = Item::pack(A[0], A[1]), VB = Item::pack(B[0], B[1]);
        int first = 0;
        for (int k = 0; k < a.nSeg; ++k) {
            R c[L], s[L];
            if constexpr (L == 2) Item::unpack(VA, A[0], A[1]), Item::unpack(VB, B[0], B[1]);
            pauliEvolveCS<SINGLE>(a, k, first, it.i, c, s);
            const bool im = a.segIm[k] != 0;
            forLanes<L>([&](auto l) { pauliEvolveRot(im, c[l], s[l], A[l], B[l]); });
            first = a.segEnd[k];
            if constexpr (L == 2) VA = Item::pack(A[0], A[1]), VB = Item::pack(B[0], B[1]);
        }
        if (a.hasPhase) {
            forLanes<L>([&](auto l) { pauliEvolveScale(pr, pi, A[l]); });
            forLanes<L>([&](auto l) { pauliEvolveScale(pr, pi, B[l]); });
        }
        it.template store<NT>(sv, A, B);
    }
}

// x == 0: psi[i] *= e^{-i angle(i)}, angle(i) the signed sum of the one segment
template <typename R, bool SINGLE, bool NT>
__global__ void k_pauli_evolve_diag(cplx<R>* sv, PauliEvolveArgs a, bitCapInt nItems)
{
    using Item = PairItem<R, -1>;
    constexpr int L = Item::L;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const R pr = (R)a.phaseRe, pi = (R)a.phaseIm;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, 0u, 0u);
        cplx<R> A[L];
        R c[L], s[L];
        it.template load<NT>(sv, A);
        pauliEvolveCS<SINGLE>(a, 0, 0, it.i, c, s);
        forLanes<L>([&](auto l) { s[l] = -s[l]; });
        forLanes<L>([&](auto l) { pauliEvolveScale(c[l], s[l], A[l]); });
        if (a.hasPhase) {
            forLanes<L>([&](auto l) { pauliEvolveScale(pr, pi, A[l]); });
        }
        it.template store<NT>(sv, A);
    }
}

template <typename R>
void launchPauliEvolve(cplx<R>* sv, const PauliEvolveArgs& a, hipStream_t stream)
{
    // the transcendental-free kernel needs every segment to hold one term
    bool single = a.nSeg > 0;
    for (int k = 0, first = 0; k < a.nSeg; first = a.segEnd[k++]) {
        if (a.segEnd[k] - first != 1) single = false;
    }
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        liftBool(single, [&](auto sg) {
            liftBool<sizeof(R) == 4>(useNontemporal(), [&](auto nt) {
                constexpr int MODE = decltype(mode)::value;
                constexpr bool SINGLE = decltype(sg)::value, NT = decltype(nt)::value;
                const dim3 g(gridFor(nItems)), b(QA_BLOCK);
                if constexpr (MODE < 0) {
                    hipLaunchKernelGGL((k_pauli_evolve_diag<R, SINGLE, NT>), g, b, 0, stream, sv, a, nItems);
                } else {
                    hipLaunchKernelGGL(
                        (k_pauli_evolve<R, MODE, SINGLE, NT>), g, b, 0, stream, sv, a, nItems, topPow);
                }
            });
        });
    });
}

// ---- Pauli brakets, H|psi>, fused adjoint step ------------------------------------
//
// With W(i) = wr(i) + i wi(i) the summed weight of a group at index i, the
// partner's weight is conj(W(i)): a term of the re set has an even number of
// Y factors, popcount(x & z) is even and its sign is the same at i and i^x;
// a term of the im set has an odd number and its sign flips. No second
// popcount over the index is needed.

// pair (i, j): W conj(q) a + conj(W) conj(p) b, with a = psi[i], b = psi[j],
// p = bra[i], q = bra[j] and W = wr + i wi; products in R, sums in double
template <typename R>
__device__ __forceinline__ void pauliBraketPair(cplx<R> a, cplx<R> b, cplx<R> p, cplx<R> q, double wr, double wi,
    double& re, double& im)
{
    const R t1r = q.re * a.re + q.im * a.im, t1i = q.re * a.im - q.im * a.re;
    const R t2r = p.re * b.re + p.im * b.im, t2i = p.re * b.im - p.im * b.re;
    re += wr * ((double)t1r + (double)t2r) - wi * ((double)t1i - (double)t2i);
    im += wr * ((double)t1i + (double)t2i) + wi * ((double)t1r - (double)t2r);
}

// w conj(p) a: a diagonal term, and the identity's share of any pair
template <typename R>
__device__ __forceinline__ void pauliBraketDiag(cplx<R> a, cplx<R> p, double w, double& re, double& im)
{
    re += w * (double)(p.re * a.re + p.im * a.im);
    im += w * (double)(p.re * a.im - p.im * a.re);
}

// <bra| sum_t c_t P_t |psi> for one group with x != 0, plus ident <bra|psi>
template <typename R, int MODE>
__global__ void k_pauli_braket(const cplx<R>* psi, const cplx<R>* bra, PauliArgs a, double ident,
    bitCapInt nItems, bitCapInt topPow, double* partialsRe, double* partialsIm)
{
    using Item = PairItem<R, MODE>;
    constexpr int L = Item::L;
    double re = 0, im = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, topPow, a.x);
        cplx<R> A[L], B[L], P[L], Q[L];
        double wr[L], wi[L];
        it.load(psi, A, B);
        it.load(bra, P, Q);
        pauliWeights(a, 0, a.nRe, it.i, wr);
        pauliWeights(a, a.nRe, a.nTerms, it.i, wi);
        forLanes<L>([&](auto l) { pauliBraketPair(A[l], B[l], P[l], Q[l], wr[l], wi[l], re, im); });
        if (ident != 0) {
            forLanes<L>([&](auto l) { pauliBraketDiag(A[l], P[l], ident, re, im); });
            forLanes<L>([&](auto l) { pauliBraketDiag(B[l], Q[l], ident, re, im); });
        }
    }
    blockSumStore2(re, im, partialsRe + blockIdx.x, partialsIm + blockIdx.x);
}

// x == 0: sum_i (ident + sum_t c_t (-1)^popcount(i&z_t)) conj(bra[i]) psi[i]
template <typename R>
__global__ void k_pauli_braket_diag(const cplx<R>* psi, const cplx<R>* bra, PauliArgs a, double ident,
    bitCapInt nItems, double* partialsRe, double* partialsIm)
{
    using Item = PairItem<R, -1>;
    constexpr int L = Item::L;
    double re = 0, im = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, 0u, 0u);
        cplx<R> A[L], P[L];
        double w[L];
        it.load(psi, A);
        it.load(bra, P);
        pauliWeights(a, 0, a.nTerms, it.i, w);
        forLanes<L>([&](auto l) { pauliBraketDiag(A[l], P[l], w[l] + ident, re, im); });
    }
    blockSumStore2(re, im, partialsRe + blockIdx.x, partialsIm + blockIdx.x);
}

template <typename R>
void launchPauliBraket(const cplx<R>* psi, const cplx<R>* bra, const PauliArgs& a, double ident,
    double* partialsDev, double* resultDev, hipStream_t stream)
{
    double* pRe = partialsDev;
    double* pIm = partialsDev + QA_REDUCE_MAX_BLOCKS;
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        constexpr int MODE = decltype(mode)::value;
        const int grid = gridForPairs(nItems);
        const dim3 g(grid), b(QA_BLOCK);
        if constexpr (MODE < 0) {
            hipLaunchKernelGGL((k_pauli_braket_diag<R>), g, b, 0, stream, psi, bra, a, ident, nItems, pRe, pIm);
        } else {
            hipLaunchKernelGGL(
                (k_pauli_braket<R, MODE>), g, b, 0, stream, psi, bra, a, ident, nItems, topPow, pRe, pIm);
        }
        hipLaunchKernelGGL(k_pauli_finish2, dim3(1), b, 0, stream, pRe, pIm, grid, resultDev);
    });
}

// d <- d + (wr + i wi) a, everything in R
template <typename R> __device__ __forceinline__ void pauliApplyMad(R wr, R wi, cplx<R> a, cplx<R>& d)
{
    d.re += wr * a.re - wi * a.im;
    d.im += wr * a.im + wi * a.re;
}

// d <- d - c p for one amplitude a of u, and the share - c Re(conj(a) p) of A
template <typename R>
__device__ __forceinline__ void krylovPrev(cplx<R> a, cplx<R> p, R c, double cd, cplx<R>& d, double& s)
{
    d.re -= c * p.re;
    d.im -= c * p.im;
    s -= cd * (double)(a.re * p.re + a.im * p.im);
}

// One item of dest (+)= (sum_t c_t P_t) psi for a group with x != 0: dest[i]
// takes W(j) psi[j] and dest[j] takes W(i) psi[i]. FIRST: dest is written
// without being read, and ident * psi rides along (psi[i] and psi[j] are in
// registers). KRYLOV (k_krylov_apply, below) adds to s the pair's share
// 2 Re(W conj(psi[j]) psi[i]) + ident (|psi[i]|^2 + |psi[j]|^2) of Re <psi|dest>
// and, when FIRST, takes - bcoef * prev from a third stream (prev == nullptr:
// none).
template <typename R, int MODE, bool FIRST, bool KRYLOV>
__device__ __forceinline__ void pauliApplyItem(const cplx<R>* psi, const cplx<R>* prev, cplx<R>* dest,
    const PauliArgs& a, double ident, double bcoef, bitCapInt v, bitCapInt topPow, double& s)
{
    using Item = PairItem<R, MODE>;
    constexpr int L = Item::L;
    const Item it(v, topPow, a.x);
    cplx<R> A[L], B[L], DA[L], DB[L];
    double wr[L], wi[L];
    it.load(psi, A, B);
    pauliWeights(a, 0, a.nRe, it.i, wr);
    pauliWeights(a, a.nRe, a.nTerms, it.i, wi);
    if constexpr (KRYLOV) {
        forLanes<L>([&](auto l) { s += pauliPair(A[l], B[l], wr[l], wi[l]); });
    }
    if constexpr (FIRST) {
        const R id = (R)ident;
        forLanes<L>([&](auto l) {
            DA[l] = cplx<R>(id * A[l].re, id * A[l].im);
            DB[l] = cplx<R>(id * B[l].re, id * B[l].im);
        });
        if constexpr (KRYLOV) {
            s += ident * (pauliLaneNorm(A) + pauliLaneNorm(B));
            if (prev) {
                const R bc = (R)bcoef;
                cplx<R> P[L], Q[L];
                it.load(prev, P, Q);
                forLanes<L>([&](auto l) { krylovPrev(A[l], P[l], bc, bcoef, DA[l], s); });
                forLanes<L>([&](auto l) { krylovPrev(B[l], Q[l], bc, bcoef, DB[l], s); });
            }
        }
    } else {
        it.load(dest, DA, DB);
    }
    forLanes<L>([&](auto l) { pauliApplyMad((R)wr[l], -(R)wi[l], B[l], DA[l]); });
    forLanes<L>([&](auto l) { pauliApplyMad((R)wr[l], (R)wi[l], A[l], DB[l]); });
    it.store(dest, DA, DB);
}

// x == 0: dest[i] (+)= W(i) psi[i] with W(i) = sum_t c_t (-1)^popcount(i&z_t),
// plus ident when FIRST; KRYLOV's share is W(i) |psi[i]|^2
template <typename R, bool FIRST, bool KRYLOV>
__device__ __forceinline__ void pauliApplyDiagItem(const cplx<R>* psi, const cplx<R>* prev, cplx<R>* dest,
    const PauliArgs& a, double ident, double bcoef, bitCapInt v, double& s)
{
    using Item = PairItem<R, -1>;
    constexpr int L = Item::L;
    const Item it(v, 0u, 0u);
    cplx<R> A[L], D[L];
    double w[L];
    it.load(psi, A);
    pauliWeights(a, 0, a.nTerms, it.i, w);
    if constexpr (FIRST) {
        forLanes<L>([&](auto l) { w[l] += ident; });
    }
    if constexpr (KRYLOV) {
        s += pauliLaneWeightedNorm(w, A);
    }
    if constexpr (FIRST) {
        forLanes<L>([&](auto l) { D[l] = cplx<R>((R)w[l] * A[l].re, (R)w[l] * A[l].im); });
        if constexpr (KRYLOV) {
            if (prev) {
                const R bc = (R)bcoef;
                cplx<R> P[L];
                it.load(prev, P);
                forLanes<L>([&](auto l) { krylovPrev(A[l], P[l], bc, bcoef, D[l], s); });
            }
        }
    } else {
        it.load(dest, D);
        forLanes<L>([&](auto l) {
            D[l].re += (R)w[l] * A[l].re;
            D[l].im += (R)w[l] * A[l].im;
        });
    }
    it.store(dest, D);
}

template <typename R, int MODE, bool FIRST>
__global__ void k_pauli_apply(const cplx<R>* psi, cplx<R>* dest, PauliArgs a, double ident,
    bitCapInt nItems, bitCapInt topPow)
{
    double unused = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        pauliApplyItem<R, MODE, FIRST, false>(psi, nullptr, dest, a, ident, 0.0, v, topPow, unused);
    }
}

template <typename R, bool FIRST>
__global__ void k_pauli_apply_diag(const cplx<R>* psi, cplx<R>* dest, PauliArgs a, double ident, bitCapInt nItems)
{
    double unused = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        pauliApplyDiagItem<R, FIRST, false>(psi, nullptr, dest, a, ident, 0.0, v, unused);
    }
}

template <typename R>
void launchPauliApply(const cplx<R>* psi, cplx<R>* dest, const PauliArgs& a, double ident, bool first,
    hipStream_t stream)
{
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        liftBool(first, [&](auto fs) {
            constexpr int MODE = decltype(mode)::value;
            constexpr bool FIRST = decltype(fs)::value;
            const double id = FIRST ? ident : 0.0;
            const dim3 g(gridForPairs(nItems)), b(QA_BLOCK);
            if constexpr (MODE < 0) {
                hipLaunchKernelGGL((k_pauli_apply_diag<R, FIRST>), g, b, 0, stream, psi, dest, a, id, nItems);
            } else {
                hipLaunchKernelGGL(
                    (k_pauli_apply<R, MODE, FIRST>), g, b, 0, stream, psi, dest, a, id, nItems, topPow);
            }
        });
    });
}

// p[l]: parity of (i + l) & z, the sign of the one string at that index
template <int L> __device__ __forceinline__ void pauliAdjointParity(bitCapInt z, bitCapInt i, unsigned (&p)[L])
{
    p[0] = __popcll(i & z) & 1u;
    if constexpr (L == 2) p[1] = p[0] ^ (unsigned)(z & 1u);
}

// One step of the adjoint sweep for a trainable rotation exp(-i theta P): sum
// <lam|P|psi> over the pairs, then apply exp(+i theta P) to both vectors while
// their amplitudes are in registers. P commutes with the rotation, so the sum
// has the same value before and after. The host supplies cos and sin of the
// angle (the SINGLE path of k_pauli_evolve): no device transcendental.
template <typename R, int MODE, bool NT>
__global__ void k_pauli_adjoint(cplx<R>* psi, cplx<R>* lam, PauliAdjointArgs a, bitCapInt nItems,
    bitCapInt topPow, double* partialsRe, double* partialsIm)
{
    using Item = PairItem<R, MODE>;
    constexpr int L = Item::L;
    double re = 0, im = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const bool isIm = a.im != 0;
    const R c = (R)a.cs, s = (R)a.sn;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, topPow, a.x);
        cplx<R> A[L], B[L], P[L], Q[L];
        unsigned p[L];
        double w[L];
        R sl[L];
        it.template load<NT>(psi, A, B);
        it.template load<NT>(lam, P, Q);
        pauliAdjointParity(a.z, it.i, p);
        forLanes<L>([&](auto l) { w[l] = p[l] ? -a.w : a.w; });
        forLanes<L>([&](auto l) {
            pauliBraketPair(A[l], B[l], P[l], Q[l], isIm ? 0.0 : w[l], isIm ? w[l] : 0.0, re, im);
        });
        forLanes<L>([&](auto l) { sl[l] = p[l] ? -s : s; });
        forLanes<L>([&](auto l) { pauliEvolveRot(isIm, c, sl[l], A[l], B[l]); });
        forLanes<L>([&](auto l) { pauliEvolveRot(isIm, c, sl[l], P[l], Q[l]); });
        it.template store<NT>(psi, A, B);
        it.template store<NT>(lam, P, Q);
    }
    blockSumStore2(re, im, partialsRe + blockIdx.x, partialsIm + blockIdx.x);
}

// x == 0: the string is diagonal; both vectors are multiplied by e^{-i angle(i)}
template <typename R, bool NT>
__global__ void k_pauli_adjoint_diag(cplx<R>* psi, cplx<R>* lam, PauliAdjointArgs a, bitCapInt nItems,
    double* partialsRe, double* partialsIm)
{
    using Item = PairItem<R, -1>;
    constexpr int L = Item::L;
    double re = 0, im = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    const R c = (R)a.cs, s = (R)a.sn;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        const Item it(v, 0u, 0u);
        cplx<R> A[L], P[L];
        unsigned p[L];
        R sl[L];
        it.template load<NT>(psi, A);
        it.template load<NT>(lam, P);
        pauliAdjointParity(a.z, it.i, p);
        forLanes<L>([&](auto l) {
            pauliBraketDiag(A[l], P[l], p[l] ? -a.w : a.w, re, im);
            sl[l] = p[l] ? s : -s; // minus the pair kernel's signed sine: e^{-i angle}
        });
        forLanes<L>([&](auto l) { pauliEvolveScale(c, sl[l], A[l]); });
        forLanes<L>([&](auto l) { pauliEvolveScale(c, sl[l], P[l]); });
        it.template store<NT>(psi, A);
        it.template store<NT>(lam, P);
    }
    blockSumStore2(re, im, partialsRe + blockIdx.x, partialsIm + blockIdx.x);
}

template <typename R>
void launchPauliAdjoint(cplx<R>* psi, cplx<R>* lam, const PauliAdjointArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream)
{
    double* pRe = partialsDev;
    double* pIm = partialsDev + QA_REDUCE_MAX_BLOCKS;
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        liftBool<sizeof(R) == 4>(useNontemporal(), [&](auto nt) {
            constexpr int MODE = decltype(mode)::value;
            constexpr bool NT = decltype(nt)::value;
            const int grid = gridForPairs(nItems);
            const dim3 g(grid), b(QA_BLOCK);
            if constexpr (MODE < 0) {
                hipLaunchKernelGGL((k_pauli_adjoint_diag<R, NT>), g, b, 0, stream, psi, lam, a, nItems, pRe, pIm);
            } else {
                hipLaunchKernelGGL(
                    (k_pauli_adjoint<R, MODE, NT>), g, b, 0, stream, psi, lam, a, nItems, topPow, pRe, pIm);
            }
            hipLaunchKernelGGL(k_pauli_finish2, dim3(1), b, 0, stream, pRe, pIm, grid, resultDev);
        });
    });
}

// ---- Krylov: fused Lanczos step, basis combination ----------------------------------
//
// One Lanczos step (krylov.hpp) on the unnormalised basis is
//   w = s H u - b prev,  A = Re <u|w>,  w <- w - s^2 A u,  ||w||^2
// with s and b folded into the weight table, ident and bcoef by the host. The
// apply kernels are the KRYLOV form of k_pauli_apply's item: every pair adds
// its share of A as a double partial (both amplitudes are in registers
// already), and the FIRST form also takes - bcoef * prev.
// Each launch's block partials fold on the device into a slot of its own;
// k_krylov_finish reads the slots back, so A never visits the host before w is
// final. No atomics anywhere: every sum has a fixed order.

template <typename R, int MODE, bool FIRST>
__global__ void k_krylov_apply(const cplx<R>* u, const cplx<R>* prev, cplx<R>* dest, PauliArgs a,
    double ident, double bcoef, bitCapInt nItems, bitCapInt topPow, double* partials)
{
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        pauliApplyItem<R, MODE, FIRST, true>(u, prev, dest, a, ident, bcoef, v, topPow, s);
    }
    blockSumStore(s, partials + blockIdx.x);
}

template <typename R, bool FIRST>
__global__ void k_krylov_apply_diag(const cplx<R>* u, const cplx<R>* prev, cplx<R>* dest, PauliArgs a,
    double ident, double bcoef, bitCapInt nItems, double* partials)
{
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        pauliApplyDiagItem<R, FIRST, true>(u, prev, dest, a, ident, bcoef, v, s);
    }
    blockSumStore(s, partials + blockIdx.x);
}

template <typename R>
void launchKrylovApply(const cplx<R>* u, const cplx<R>* prev, cplx<R>* dest, const PauliArgs& a, double ident,
    double bcoef, bool first, double* partialsDev, double* slotDev, hipStream_t stream)
{
    pauliPairDispatch<R>(a.x, a.nAmps, [&](auto mode, bitCapInt nItems, bitCapInt topPow) {
        liftBool(first, [&](auto fs) {
            constexpr int MODE = decltype(mode)::value;
            constexpr bool FIRST = decltype(fs)::value;
            const cplx<R>* pv = FIRST ? prev : nullptr;
            const double id = FIRST ? ident : 0.0, bc = FIRST ? bcoef : 0.0;
            const int grid = gridForPairs(nItems);
            const dim3 g(grid), b(QA_BLOCK);
            if constexpr (MODE < 0) {
                hipLaunchKernelGGL((k_krylov_apply_diag<R, FIRST>), g, b, 0, stream, u, pv, dest, a, id, bc,
                    nItems, partialsDev);
            } else {
                hipLaunchKernelGGL((k_krylov_apply<R, MODE, FIRST>), g, b, 0, stream, u, pv, dest, a, id, bc,
                    nItems, topPow, partialsDev);
            }
            hipLaunchKernelGGL(k_pauli_finish, dim3(1), b, 0, stream, partialsDev, grid, slotDev);
        });
    });
}

// w <- w - a u with a = scale * (sum of the step's slots), and the block's
// share of ||w||^2. STORE = false (the last step of a run) only sums.
template <typename R, bool STORE>
__global__ void k_krylov_finish(const cplx<R>* u, cplx<R>* w, const double* slots, int nSlots, double scale,
    bitCapInt nItems, double* partials)
{
    double A = 0;
    for (int k = 0; k < nSlots; ++k) A += slots[k];
    const R a = (R)(scale * A);
    double s = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        if constexpr (sizeof(R) == 4) {
            const float4 U = reinterpret_cast<const float4*>(u)[v];
            float4 W = reinterpret_cast<float4*>(w)[v];
            W.x -= a * U.x;
            W.y -= a * U.y;
            W.z -= a * U.z;
            W.w -= a * U.w;
            if constexpr (STORE) reinterpret_cast<float4*>(w)[v] = W;
            s += (double)(W.x * W.x + W.y * W.y) + (double)(W.z * W.z + W.w * W.w);
        } else {
            const double2 U = reinterpret_cast<const double2*>(u)[v];
            double2 W = reinterpret_cast<double2*>(w)[v];
            W.x -= a * U.x;
            W.y -= a * U.y;
            if constexpr (STORE) reinterpret_cast<double2*>(w)[v] = W;
            s += W.x * W.x + W.y * W.y;
        }
    }
    blockSumStore(s, partials + blockIdx.x);
}

// stage 2 of the finish: result[0] = sum of the slots, result[1] = ||w||^2
__global__ void k_krylov_fold(const double* partials, int n, const double* slots, int nSlots, double* result)
{
    double s = 0;
    for (int k = threadIdx.x; k < n; k += QA_BLOCK) s += partials[k];
    blockSumStore(s, result + 1);
    if (threadIdx.x == 0) {
        double A = 0;
        for (int k = 0; k < nSlots; ++k) A += slots[k];
        result[0] = A;
    }
}

template <typename R>
void launchKrylovFinish(const cplx<R>* u, cplx<R>* w, bitCapInt nAmps, const double* slotsDev, int nSlots,
    double scale, bool store, double* partialsDev, double* resultDev, hipStream_t stream)
{
    const bitCapInt nItems = (sizeof(R) == 4) ? (nAmps >> 1u) : nAmps;
    const int grid = gridForPairs(nItems);
    const dim3 g(grid), b(QA_BLOCK);
    if (store) {
        hipLaunchKernelGGL((k_krylov_finish<R, true>), g, b, 0, stream, u, w, slotsDev, nSlots, scale, nItems,
            partialsDev);
    } else {
        hipLaunchKernelGGL((k_krylov_finish<R, false>), g, b, 0, stream, u, w, slotsDev, nSlots, scale, nItems,
            partialsDev);
    }
    hipLaunchKernelGGL(
        k_krylov_fold, dim3(1), dim3(QA_BLOCK), 0, stream, partialsDev, grid, slotsDev, nSlots, resultDev);
}

// (re, im) += (cr + i ci) (ur + i ui)
template <typename R> __device__ __forceinline__ void krylovMad(R cr, R ci, R ur, R ui, R& re, R& im)
{
    re += cr * ur - ci * ui;
    im += cr * ui + ci * ur;
}

// state <- coef[0] state + sum_j coef[j + 1] src[j]: elementwise, so in place
// is safe. Pointers and coefficients ride in the kernel arguments.
template <typename R>
__global__ void k_krylov_combine(cplx<R>* state, KrylovCombineArgs<R> a, bitCapInt nItems)
{
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        if constexpr (sizeof(R) == 4) {
            const float4 S = reinterpret_cast<float4*>(state)[v];
            float4 D = make_float4(0.f, 0.f, 0.f, 0.f);
            krylovMad<float>((float)a.coefRe[0], (float)a.coefIm[0], S.x, S.y, D.x, D.y);
            krylovMad<float>((float)a.coefRe[0], (float)a.coefIm[0], S.z, S.w, D.z, D.w);
            for (int j = 0; j < a.nSrc; ++j) {
                const float4 U = reinterpret_cast<const float4*>(a.src[j])[v];
                const float cr = (float)a.coefRe[j + 1], ci = (float)a.coefIm[j + 1];
                krylovMad<float>(cr, ci, U.x, U.y, D.x, D.y);
                krylovMad<float>(cr, ci, U.z, U.w, D.z, D.w);
            }
            reinterpret_cast<float4*>(state)[v] = D;
        } else {
            const double2 S = reinterpret_cast<double2*>(state)[v];
            double2 D = make_double2(0.0, 0.0);
            krylovMad<double>(a.coefRe[0], a.coefIm[0], S.x, S.y, D.x, D.y);
            for (int j = 0; j < a.nSrc; ++j) {
                const double2 U = reinterpret_cast<const double2*>(a.src[j])[v];
                krylovMad<double>(a.coefRe[j + 1], a.coefIm[j + 1], U.x, U.y, D.x, D.y);
            }
            reinterpret_cast<double2*>(state)[v] = D;
        }
    }
}

template <typename R>
void launchKrylovCombine(cplx<R>* state, bitCapInt nAmps, const KrylovCombineArgs<R>& a, hipStream_t stream)
{
    const bitCapInt nItems = (sizeof(R) == 4) ? (nAmps >> 1u) : nAmps;
    hipLaunchKernelGGL(
        (k_krylov_combine<R>), dim3(gridForPairs(nItems)), dim3(QA_BLOCK), 0, stream, state, a, nItems);
}

// ---- Krylov: block orthogonalisation, basis rotation --------------------------------
//
// One launch of k_krylov_orth handles a chunk of up to 16 basis vectors u_i
// (krylov.hpp, LanczosLowestStates): with coef it first takes
//   w <- w - sum_i (scale_i coef_i) u_i,   coef_i = (coef[2i], coef[2i + 1])
// read from device memory, the folded result of an earlier launch, so that no
// coefficient visits the host between launches; then it forms <u_i|w> for
// every i and ||w||^2 of that w. Every u_i is loaded once and kept in
// registers between the two uses. Products are formed in R, sums are double.
// All per-vector arrays are indexed by fully unrolled loops under wave-uniform
// guards, so they live in registers. Each block leaves its 33 sums in
// partials[q * gridDim.x + block]; k_krylov_orth_fold adds them in a fixed
// order, one wave per sum. No atomics.

static inline int gridForOrth(bitCapInt nItems)
{
    int grid = gridForPairs(nItems);
    return grid > KRYLOV_ORTH_MAX_BLOCKS ? KRYLOV_ORTH_MAX_BLOCKS : grid;
}

int krylovOrthGrid(bitCapInt nItems) { return gridForOrth(nItems); }

// The launch bounds lift the 128-register limit of a 1024-thread block (16
// vectors and 33 double sums per thread need more, and would spill under it)
// and keep two waves on a SIMD.
template <typename R, bool STORE>
__global__ void __launch_bounds__(QA_BLOCK, 2) k_krylov_orth(
    cplx<R>* w, KrylovOrthArgs<R> a, const double* coef, bitCapInt nItems, double* partials)
{
    constexpr int N = KRYLOV_ORTH_MAX_VECTORS;
    using V = typename std::conditional<sizeof(R) == 4, float4, double2>::type;
    double accRe[N], accIm[N];
    R cr[N], ci[N];
    double nrm = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        accRe[i] = 0;
        accIm[i] = 0;
        cr[i] = 0;
        ci[i] = 0;
        if (coef && i < a.n) {
            cr[i] = (R)(a.scale[i] * coef[2 * i]);
            ci[i] = (R)(a.scale[i] * coef[2 * i + 1]);
        }
    }
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        V W = reinterpret_cast<V*>(w)[v];
        V U[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i < a.n) U[i] = reinterpret_cast<const V*>(a.u[i])[v];
        }
        if (coef) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (i < a.n) {
                    W.x -= cr[i] * U[i].x - ci[i] * U[i].y;
                    W.y -= cr[i] * U[i].y + ci[i] * U[i].x;
                    if constexpr (sizeof(R) == 4) {
                        W.z -= cr[i] * U[i].z - ci[i] * U[i].w;
                        W.w -= cr[i] * U[i].w + ci[i] * U[i].z;
                    }
                }
            }
            if constexpr (STORE) reinterpret_cast<V*>(w)[v] = W;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i < a.n) {
                if constexpr (sizeof(R) == 4) {
                    accRe[i] += (double)(U[i].x * W.x + U[i].y * W.y) + (double)(U[i].z * W.z + U[i].w * W.w);
                    accIm[i] += (double)(U[i].x * W.y - U[i].y * W.x) + (double)(U[i].z * W.w - U[i].w * W.z);
                } else {
                    accRe[i] += U[i].x * W.x + U[i].y * W.y;
                    accIm[i] += U[i].x * W.y - U[i].y * W.x;
                }
            }
        }
        if constexpr (sizeof(R) == 4) {
            nrm += (double)(W.x * W.x + W.y * W.y) + (double)(W.z * W.z + W.w * W.w);
        } else {
            nrm += W.x * W.x + W.y * W.y;
        }
    }
    // block sums of all 33 values behind one barrier: a row of LDS per value
    constexpr int Q = KRYLOV_ORTH_RESULTS;
    __shared__ double waveSums[Q][QA_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double re = waveReduceSum(accRe[i]);
        const double im = waveReduceSum(accIm[i]);
        if (lane == 0) {
            waveSums[2 * i][wid] = re;
            waveSums[2 * i + 1][wid] = im;
        }
    }
    nrm = waveReduceSum(nrm);
    if (lane == 0) waveSums[Q - 1][wid] = nrm;
    __syncthreads();
    if (threadIdx.x < Q) {
        double t = 0;
        for (int k = 0; k < QA_BLOCK / 64; ++k) t += waveSums[threadIdx.x][k];
        partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// result[q] = sum over the blocks of partials[q * n + block], wave q % 4 of
// the one block, lanes striding the blocks: a fixed order
__global__ void k_krylov_orth_fold(const double* partials, int n, double* result)
{
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < KRYLOV_ORTH_RESULTS; q += QA_BLOCK / 64) {
        double s = 0;
        for (int b = lane; b < n; b += 64) s += partials[(size_t)q * n + b];
        s = waveReduceSum(s);
        if (lane == 0) result[q] = s;
    }
}

template <typename R>
void launchKrylovOrth(cplx<R>* w, bitCapInt nAmps, const KrylovOrthArgs<R>& a, const double* coefDev,
    bool store, double* partialsDev, double* resultDev, hipStream_t stream)
{
    const bitCapInt nItems = (sizeof(R) == 4) ? (nAmps >> 1u) : nAmps;
    const int grid = gridForOrth(nItems);
    const dim3 g(grid), b(QA_BLOCK);
    if (store && coefDev) {
        hipLaunchKernelGGL((k_krylov_orth<R, true>), g, b, 0, stream, w, a, coefDev, nItems, partialsDev);
    } else {
        hipLaunchKernelGGL((k_krylov_orth<R, false>), g, b, 0, stream, w, a, coefDev, nItems, partialsDev);
    }
    hipLaunchKernelGGL(k_krylov_orth_fold, dim3(1), dim3(QA_BLOCK), 0, stream, partialsDev, grid, resultDev);
}

// The restart: out_i = sum_r m[r * 16 + i] in_r for i < kp, r < k, with the
// real matrix (rows padded to 16, the basis's scales folded in by the host)
// read wave-uniformly from device memory. A thread reads its element of every
// input before it writes its element of the outputs, so an output may be one
// of the inputs' buffers. The kp accumulators stay in registers.
template <typename R> __global__ void k_krylov_rotate(KrylovRotateArgs<R> a, const R* m, bitCapInt nItems)
{
    constexpr int N = KRYLOV_COMBINE_MAX_VECTORS;
    using V = typename std::conditional<sizeof(R) == 4, float4, double2>::type;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < nItems; v += stride) {
        V acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if constexpr (sizeof(R) == 4) {
                acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                acc[i] = make_double2(0.0, 0.0);
            }
        }
        for (int r = 0; r < a.k; ++r) {
            const V U = reinterpret_cast<const V*>(a.in[r])[v];
            const R* row = m + r * N;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (i < a.kp) {
                    const R c = row[i];
                    acc[i].x += c * U.x;
                    acc[i].y += c * U.y;
                    if constexpr (sizeof(R) == 4) {
                        acc[i].z += c * U.z;
                        acc[i].w += c * U.w;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i < a.kp) reinterpret_cast<V*>(a.out[i])[v] = acc[i];
        }
    }
}

template <typename R>
void launchKrylovRotate(const KrylovRotateArgs<R>& a, const R* mDev, bitCapInt nAmps, hipStream_t stream)
{
    const bitCapInt nItems = (sizeof(R) == 4) ? (nAmps >> 1u) : nAmps;
    hipLaunchKernelGGL(
        (k_krylov_rotate<R>), dim3(gridForPairs(nItems)), dim3(QA_BLOCK), 0, stream, a, mDev, nItems);
}

// ---- reduced density matrices -----------------------------------------------------
//
// rho[a,b] = sum_e psi[e,a] conj(psi[e,b]) over the kept qubits in ascending
// physical order (the engine permutes into the caller's order). Read-only:
// every launch leaves one set of double partials per block, and k_rdm_fold
// adds the sets in a fixed order. Products are formed in R; sums are double,
// but for runs of at most QA_RDM_RUN rows in the tile kernel.

// deposit the low bits of x at the set bits of mask, lowest first
__device__ __forceinline__ bitCapInt rdmDeposit(bitCapInt x, bitCapInt mask)
{
    bitCapInt r = 0;
    while (mask) {
        const bitCapInt low = mask & (~mask + 1u);
        if (x & 1u) r |= low;
        x >>= 1u;
        mask ^= low;
    }
    return r;
}

// one environment row into the packed triangle: entry (a, b > a) keeps its
// real part at [a*D+b] and its imaginary part at [b*D+a]
template <typename R, int D>
__device__ __forceinline__ void rdmRowAdd(const R (&re)[D], const R (&im)[D], double (&acc)[D * D])
{
#pragma unroll
    for (int a = 0; a < D; ++a) {
        acc[a * D + a] += (double)(re[a] * re[a] + im[a] * im[a]);
#pragma unroll
        for (int b = a + 1; b < D; ++b) {
            acc[a * D + b] += (double)(re[a] * re[b] + im[a] * im[b]);
            acc[b * D + a] += (double)(im[a] * re[b] - re[a] * im[b]);
        }
    }
}

// Register regime. MODE 0: fp64, one row per item; 1: fp32, qubit 0 in the
// environment, a 16-byte load holds the same entry of two rows; 2: fp32, qubit
// 0 kept, a load holds entries a and a+1 of one row (as k_pauli_group MODE 2)
template <typename R, int K, int MODE>
__global__ __launch_bounds__(QA_BLOCK) void k_rdm_reg(const cplx<R>* sv, RdmRegArgs a, double* partials)
{
    constexpr int D = 1 << K;
    double acc[D * D];
#pragma unroll
    for (int t = 0; t < D * D; ++t) acc[t] = 0;
    const bitCapInt stride = (bitCapInt)gridDim.x * blockDim.x;
    for (bitCapInt v = (bitCapInt)blockIdx.x * blockDim.x + threadIdx.x; v < a.nItems; v += stride) {
        bitCapInt i = (MODE == 1) ? (v << 1u) : v;
#pragma unroll
        for (int j = 0; j < K; ++j) i = ((i & ~(a.pows[j] - 1u)) << 1u) | (i & (a.pows[j] - 1u));
        if constexpr (MODE == 0) {
            R re[D], im[D];
#pragma unroll
            for (int x = 0; x < D; ++x) {
                const double2 A = reinterpret_cast<const double2*>(sv)[i | a.off[x]];
                re[x] = A.x;
                im[x] = A.y;
            }
            rdmRowAdd<R, D>(re, im, acc);
        } else if constexpr (MODE == 1) {
            R re0[D], im0[D], re1[D], im1[D];
#pragma unroll
            for (int x = 0; x < D; ++x) {
                const float4 A = reinterpret_cast<const float4*>(sv)[(i | a.off[x]) >> 1u];
                re0[x] = A.x;
                im0[x] = A.y;
                re1[x] = A.z;
                im1[x] = A.w;
            }
            rdmRowAdd<R, D>(re0, im0, acc);
            rdmRowAdd<R, D>(re1, im1, acc);
        } else {
            R re[D], im[D];
#pragma unroll
            for (int x = 0; x < D; x += 2) {
                const float4 A = reinterpret_cast<const float4*>(sv)[(i | a.off[x]) >> 1u];
                re[x] = A.x;
                im[x] = A.y;
                re[x + 1] = A.z;
                im[x + 1] = A.w;
            }
            rdmRowAdd<R, D>(re, im, acc);
        }
    }
    // block fold in a fixed order: wave shuffle -> LDS -> one set of D*D doubles
    __shared__ double waveSums[QA_BLOCK / 64][D * D];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < D * D; ++t) {
        const double s = waveReduceSum(acc[t]);
        if (lane == 0) waveSums[wid][t] = s;
    }
    __syncthreads();
    if (threadIdx.x < D * D) {
        double s = 0;
        for (int w = 0; w < QA_BLOCK / 64; ++w) s += waveSums[w][threadIdx.x];
        partials[(size_t)blockIdx.x * (D * D) + threadIdx.x] = s;
    }
}

// Tile regime. The tile lies in LDS in physical address order, so the load is
// a plain copy in 16-byte vectors; the kept bits are picked out when the
// patches read it. A thread owns the 4x4 patch (pa, pb) of the KT-bit block
// and, where there are fewer patches than threads, one of G row groups.
// DIAG (row and column side are the same slice): only the patches with
// pa <= pb exist, numbered row by row; the host mirrors the rest.
// Partials: entry f = r * P + p of a block's set, r = (i*4 + j)*2 + (0: re,
// 1: im) inside patch p (pa * (DT/4) + pb when every patch exists).
//
// Kept bits high in the tile put the patches of a wave whole rows apart, all
// on one bank, so the low index bits are XOR-ed with the next ones (the QFT
// tiles' swizzle). The map is linear over XOR, and a row index and a kept
// offset share no bit: swz(row | off) = swz(row) ^ swz(off). Bit 0 stays, so
// an fp32 pair still moves as one 16-byte vector.
template <typename R> __device__ __forceinline__ uint32_t rdmSwz(uint32_t x)
{
    return (sizeof(R) == 4) ? (x ^ ((x >> 6) & 62u)) : (x ^ ((x >> 5) & 31u));
}

template <typename R, int KT, bool DIAG>
__global__ __launch_bounds__(QA_BLOCK) void k_rdm_tile(const cplx<R>* sv, RdmTileArgs a, double* partials)
{
    static_assert(QA_BLOCK == 256, "patch layout assumes 256 threads");
    using V = typename std::conditional<sizeof(R) == 4, float4, double2>::type;
    using C = typename std::conditional<sizeof(R) == 4, float2, double2>::type;
    constexpr int APV = (sizeof(R) == 4) ? 2 : 1; // amplitudes per 16-byte vector
    constexpr int LB = (sizeof(R) == 4) ? 9 : 8;  // tile-index bits a block covers per trip
    constexpr int DT = 1 << KT;
    constexpr int NP = DT / 4;
    constexpr int P = rdmTilePatches(KT, DIAG);
    constexpr int G = QA_BLOCK / P;
    extern __shared__ __attribute__((aligned(16))) unsigned char rdmLds[];
    const int T = a.tileAddrBits;
    const uint32_t tileAmps = 1u << T;
    const C* tileA = reinterpret_cast<const C*>(rdmLds);
    const C* tileB = DIAG ? tileA : tileA + tileAmps;
    V* ldsA = reinterpret_cast<V*>(rdmLds);
    V* ldsB = ldsA + tileAmps / APV;

    const int tid = threadIdx.x;
    const int p = tid % P;
    const int g = tid / P; // G, the spare threads of a block, has no rows
    int pa = p / NP, pb = p % NP;
    if constexpr (DIAG) {
        pa = 0;
        pb = p;
        while (pb >= NP - pa) { // row pa of the triangle has NP - pa patches
            pb -= NP - pa;
            ++pa;
        }
        pb += pa;
    }
    const uint32_t M = a.keptInTile;
    const uint32_t EM = (tileAmps - 1u) & ~M;
    uint32_t aOff[4], bOff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        aOff[i] = rdmSwz<R>((uint32_t)rdmDeposit((bitCapInt)(pa * 4 + i), M));
        bOff[i] = rdmSwz<R>((uint32_t)rdmDeposit((bitCapInt)(pb * 4 + i), M));
    }
    // group g takes rows [E g / G, E (g + 1) / G)
    const int E = 1 << (T - KT);
    const int rowLo = (g < G) ? E * g / G : E;
    const int rowsPer = (g < G) ? E * (g + 1) / G - rowLo : 0;
    const uint32_t rowStart = (uint32_t)rdmDeposit((bitCapInt)rowLo, EM);
    const bitCapInt physTid = rdmDeposit((bitCapInt)(tid * APV), a.tileMask);
    const uint32_t nVec = tileAmps / APV;

    double acc[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[r] = 0;

    for (bitCapInt tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        const bitCapInt base = rdmDeposit(tile, a.enumMask);
        __syncthreads(); // the last tile's readers are done
        for (uint32_t v0 = 0; v0 < nVec; v0 += QA_BLOCK) {
            const uint32_t v = v0 + tid;
            if (v < nVec) {
                // v0 * APV has no bit below LB, tid * APV none at or above it
                const bitCapInt phys
                    = base | physTid | rdmDeposit((bitCapInt)(v0 * APV) >> LB, a.tileMaskHigh);
                const uint32_t sw = rdmSwz<R>(v * APV) / APV;
                ldsA[sw] = reinterpret_cast<const V*>(sv)[(phys | a.rowOff) / APV];
                if constexpr (!DIAG) ldsB[sw] = reinterpret_cast<const V*>(sv)[(phys | a.colOff) / APV];
            }
        }
        __syncthreads();
        if (rowsPer > 0) {
            uint32_t idx = rowStart;
            for (int r0 = 0; r0 < rowsPer; r0 += QA_RDM_RUN) {
                R run[32];
#pragma unroll
                for (int r = 0; r < 32; ++r) run[r] = 0;
                const int rn = min(QA_RDM_RUN, rowsPer - r0);
                for (int row = 0; row < rn; ++row) {
                    C av[4], bv[4];
                    const uint32_t si = rdmSwz<R>(idx);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        av[i] = tileA[si ^ aOff[i]];
                        bv[i] = tileB[si ^ bOff[i]];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            run[(i * 4 + j) * 2] += av[i].x * bv[j].x + av[i].y * bv[j].y;
                            run[(i * 4 + j) * 2 + 1] += av[i].y * bv[j].x - av[i].x * bv[j].y;
                        }
                    }
                    idx = ((idx | ~EM) + 1u) & EM; // next row: carry across the kept bits
                }
#pragma unroll
                for (int r = 0; r < 32; ++r) acc[r] += (double)run[r];
            }
        }
    }

    double* dst = partials + (size_t)blockIdx.x * (32 * P);
    if constexpr (G == 1) {
        if (tid < P) {
#pragma unroll
            for (int r = 0; r < 32; ++r) dst[r * P + p] = acc[r];
        }
    } else {
        // the row groups add up in group order, in LDS
        double* sh = reinterpret_cast<double*>(rdmLds);
        for (int gg = 0; gg < G; ++gg) {
            __syncthreads();
            if (g == gg) {
#pragma unroll
                for (int r = 0; r < 32; ++r) sh[r * P + p] = (gg ? sh[r * P + p] : 0.0) + acc[r];
            }
        }
        __syncthreads();
        for (int f = tid; f < 32 * P; f += QA_BLOCK) dst[f] = sh[f];
    }
}

// fold nSets sets of nEntries doubles in a fixed order: a wave takes 64
// entries and a quarter of the sets, the four quarters add up in LDS
__global__ __launch_bounds__(QA_BLOCK) void k_rdm_fold(const double* partials, int nSets, int nEntries, double* result)
{
    __shared__ double quarter[QA_BLOCK / 64][64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int lo = (int)((long)nSets * wid / (QA_BLOCK / 64));
    const int hi = (int)((long)nSets * (wid + 1) / (QA_BLOCK / 64));
    double s = 0;
    if (e < nEntries) {
        for (int k = lo; k < hi; ++k) s += partials[(size_t)k * nEntries + e];
    }
    quarter[wid][lane] = s;
    __syncthreads();
    if (wid == 0 && e < nEntries) {
        double t = 0;
        for (int w = 0; w < QA_BLOCK / 64; ++w) t += quarter[w][lane];
        result[e] = t;
    }
}

static inline int rdmGrid(bitCapInt blocks, int hardCap)
{
    bitCapInt b = std::min<bitCapInt>(blocks, (bitCapInt)hardCap);
    const int cap = maxBlocks();
    if (cap > 0 && b > (bitCapInt)cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

int rdmRegGrid(bitCapInt nItems) { return rdmGrid((nItems + QA_BLOCK - 1) / QA_BLOCK, QA_RDM_REG_GRID); }
int rdmTileGrid(bitCapInt nTiles) { return rdmGrid(nTiles, QA_RDM_TILE_GRID); }

static void launchRdmFold(const double* partialsDev, int nSets, int nEntries, double* resultDev,
    hipStream_t stream)
{
    hipLaunchKernelGGL(k_rdm_fold, dim3((nEntries + 63) / 64), dim3(QA_BLOCK), 0, stream,
        partialsDev, nSets, nEntries, resultDev);
}

template <typename R>
void launchRdmReg(const cplx<R>* sv, int k, bool keepsBit0, const RdmRegArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream)
{
    const int grid = rdmRegGrid(a.nItems);
    const dim3 g(grid), b(QA_BLOCK);
#define QA_RDM_REG(K)                                                                               \
    do {                                                                                            \
        if constexpr (sizeof(R) == 8) {                                                             \
            hipLaunchKernelGGL((k_rdm_reg<R, K, 0>), g, b, 0, stream, sv, a, partialsDev);          \
        } else if (keepsBit0) {                                                                     \
            hipLaunchKernelGGL((k_rdm_reg<R, K, 2>), g, b, 0, stream, sv, a, partialsDev);          \
        } else {                                                                                    \
            hipLaunchKernelGGL((k_rdm_reg<R, K, 1>), g, b, 0, stream, sv, a, partialsDev);          \
        }                                                                                           \
    } while (0)
    switch (k) {
    case 1: QA_RDM_REG(1); break;
    case 2: QA_RDM_REG(2); break;
    case 3: QA_RDM_REG(3); break;
    default: throw QrackError("launchRdmReg: no kernel for this many kept qubits");
    }
#undef QA_RDM_REG
    launchRdmFold(partialsDev, grid, 1 << (2 * k), resultDev, stream);
}

template <typename R>
void launchRdmTile(const cplx<R>* sv, int kt, const RdmTileArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream)
{
    const int grid = rdmTileGrid(a.nTiles);
    const dim3 g(grid), b(QA_BLOCK);
    const uint32_t lds = 32768u; // the tile, or two half tiles; the group fold fits inside
#define QA_RDM_TILE(KT)                                                                             \
    do {                                                                                            \
        if (a.cross) {                                                                              \
            hipLaunchKernelGGL((k_rdm_tile<R, KT, false>), g, b, lds, stream, sv, a, partialsDev);  \
        } else {                                                                                    \
            hipLaunchKernelGGL((k_rdm_tile<R, KT, true>), g, b, lds, stream, sv, a, partialsDev);   \
        }                                                                                           \
    } while (0)
    switch (kt) {
    case 4: QA_RDM_TILE(4); break;
    case 5: QA_RDM_TILE(5); break;
    case 6: QA_RDM_TILE(6); break;
    default: throw QrackError("launchRdmTile: no kernel for this many kept qubits");
    }
#undef QA_RDM_TILE
    launchRdmFold(partialsDev, grid, 32 * rdmTilePatches(kt, !a.cross), resultDev, stream);
}

// ---- explicit instantiations ---------------------------------------------------

#define QA_INSTANTIATE(R)                                                                           \
    template void launchApply2x2<R>(cplx<R>*, const GateArgs<R>&, hipStream_t);                     \
    template void launchUniformlyControlled<R>(                                                     \
        cplx<R>*, bitCapInt, bitCapInt, const bitCapInt*, int, const cplx<R>*, hipStream_t);        \
    template void launchXMask<R>(cplx<R>*, bitCapInt, bitCapInt, hipStream_t);                      \
    template void launchParityPhase<R>(cplx<R>*, bitCapInt, bitCapInt, cplx<R>, cplx<R>, hipStream_t); \
    template int launchReduce<R>(const cplx<R>*, const ReduceArgs&, int, double*, hipStream_t);     \
    template int launchArgMax<R>(const cplx<R>*, bitCapInt, double*, bitCapInt*, hipStream_t);      \
    template void launchPauliGroup<R>(const cplx<R>*, const PauliArgs&, double*, double*, hipStream_t); \
    template void launchPauliEvolve<R>(cplx<R>*, const PauliEvolveArgs&, hipStream_t);              \
    template void launchPauliBraket<R>(                                                             \
        const cplx<R>*, const cplx<R>*, const PauliArgs&, double, double*, double*, hipStream_t);   \
    template void launchPauliApply<R>(                                                              \
        const cplx<R>*, cplx<R>*, const PauliArgs&, double, bool, hipStream_t);                     \
    template void launchPauliAdjoint<R>(                                                            \
        cplx<R>*, cplx<R>*, const PauliAdjointArgs&, double*, double*, hipStream_t);                \
    template void launchKrylovApply<R>(const cplx<R>*, const cplx<R>*, cplx<R>*, const PauliArgs&,  \
        double, double, bool, double*, double*, hipStream_t);                                       \
    template void launchKrylovFinish<R>(const cplx<R>*, cplx<R>*, bitCapInt, const double*, int,    \
        double, bool, double*, double*, hipStream_t);                                               \
    template void launchKrylovCombine<R>(                                                           \
        cplx<R>*, bitCapInt, const KrylovCombineArgs<R>&, hipStream_t);                             \
    template void launchKrylovOrth<R>(cplx<R>*, bitCapInt, const KrylovOrthArgs<R>&, const double*, \
        bool, double*, double*, hipStream_t);                                                       \
    template void launchKrylovRotate<R>(const KrylovRotateArgs<R>&, const R*, bitCapInt, hipStream_t); \
    template void launchRdmReg<R>(                                                                  \
        const cplx<R>*, int, bool, const RdmRegArgs&, double*, double*, hipStream_t);               \
    template void launchRdmTile<R>(                                                                 \
        const cplx<R>*, int, const RdmTileArgs&, double*, double*, hipStream_t);                    \
    template void launchNormalize<R>(cplx<R>*, bitCapInt, cplx<R>, R, hipStream_t);                 \
    template void launchApplyM<R>(cplx<R>*, bitCapInt, bitCapInt, bitCapInt, cplx<R>, hipStream_t); \
    template void launchApplyParity<R>(cplx<R>*, bitCapInt, bitCapInt, bool, cplx<R>, hipStream_t); \
    template void launchCompose<R>(                                                                 \
        const cplx<R>*, const cplx<R>*, cplx<R>*, bitCapInt, bitLenInt, bitLenInt, hipStream_t);    \
    template void launchDisposeSlice<R>(const cplx<R>*, cplx<R>*, bitCapInt, bitLenInt, bitLenInt,  \
        bitCapInt, cplx<R>, hipStream_t);                                                           \
    template void launchGatherPart<R>(const cplx<R>*, cplx<R>*, bitCapInt, bitLenInt, bitLenInt,    \
        bitCapInt, cplx<R>, hipStream_t);                                                           \
    template void launchAllocateExpand<R>(                                                          \
        const cplx<R>*, cplx<R>*, bitCapInt, bitLenInt, bitLenInt, hipStream_t);                    \
    template void launchShuffleSwap<R>(cplx<R>*, cplx<R>*, bitCapInt, hipStream_t);                 \
    template void launchPermute<R>(const cplx<R>*, cplx<R>*, const PermArgs&, hipStream_t);         \
    template void launchCopyUncontrolled<R>(                                                        \
        const cplx<R>*, cplx<R>*, bitCapInt, bitCapInt, hipStream_t);                               \
    template void launchPhaseFlipIfLess<R>(                                                         \
        cplx<R>*, bitCapInt, bitCapInt, bitLenInt, bitCapInt, bitCapInt, hipStream_t);              \
    template void launchChunkSums<R>(const cplx<R>*, bitCapInt, bitCapInt, double*, hipStream_t);   \
    template int launchInner<R>(                                                                    \
        const cplx<R>*, const cplx<R>*, bitCapInt, double*, double*, hipStream_t);                  \
    template void launchPartProbs<R>(                                                               \
        const cplx<R>*, bitCapInt, bitLenInt, bitLenInt, double*, hipStream_t);                     \
    template void launchPhaseRamp<R>(cplx<R>*, bitCapInt, bitLenInt, bitLenInt, bitCapInt, double, hipStream_t);\
    template void launchPhaseRampGeneral<R>(cplx<R>*, bitCapInt, const RampArgs&, hipStream_t);    \
    template void launchQftColumn2<R>(cplx<R>*, bitCapInt, bitLenInt, bitLenInt, bitCapInt,        \
        bitCapInt, int, bool, hipStream_t);                                                         \
    template void launchQftColumn3<R>(cplx<R>*, bitCapInt, bitLenInt, bitLenInt, bitCapInt,        \
        bitCapInt, bitCapInt, int, bool, hipStream_t);                                              \
    template void launchQftColumnK<R>(cplx<R>*, bitCapInt, bitLenInt, bitLenInt, int,               \
        const bitCapInt*, int, bool, hipStream_t);                                                  \
    template void launchQftColumn<R>(                                                               \
        cplx<R>*, bitCapInt, bitLenInt, bitLenInt, bitCapInt, int, bool, hipStream_t);              \
    template void launchMtrx1qBatch<R>(cplx<R>*, const Batch1qArgs<R>&, hipStream_t);                               \
    template void launchCnotBatch<R>(cplx<R>*, const CnotBatchArgs&, hipStream_t);                              \
    template void launchMtrx1qBatchLds<R>(cplx<R>*, const BatchLdsArgs<R>&, hipStream_t);                \
    template void launchMtrx2qBatchLds<R>(cplx<R>*, const Batch2qLdsArgs<R>&, hipStream_t);                \
    template void launchMtrx2q<R>(cplx<R>*, const Gate4x4Args<R>&, hipStream_t);                              \
    template void launchCPhasePairs<R>(cplx<R>*, const CPhasePairsArgs&, hipStream_t);                               \
    template void launchMtrx2qPair2<R>(cplx<R>*, const Gate4x4Pair2Args<R>&, hipStream_t);         \
    template void launchQftLowLds<R>(cplx<R>*, bitCapInt, int, int, int, bool, hipStream_t);        \
    template void launchQftMidLds<R>(cplx<R>*, bitCapInt, int, int, int, bool, hipStream_t);        \
    template void launchQftLowLdsBasis<R>(                                                          \
        cplx<R>*, bitCapInt, int, int, int, bool, bitCapInt, cplx<R>, hipStream_t);                 \
    template void launchQftLowLdsSums<R>(cplx<R>*, bitCapInt, int, int, double*, hipStream_t);      \
    template void launchQftMidLdsBasis<R>(                                                          \
        cplx<R>*, bitCapInt, int, int, int, bool, bitCapInt, cplx<R>, hipStream_t);                 \
    template void launchSetAmp<R>(cplx<R>*, bitCapInt, cplx<R>, hipStream_t);                       \
    template void launchQftColumn2General<R>(cplx<R>*, bitCapInt, bitCapInt, bitCapInt,            \
        const RampArgs&, double, double, bool, hipStream_t);                                        \
    template void launchQftColumnTopRange<R>(cplx<R>*, bitCapInt, const RampArgs&, double, bool,    \
        bitCapInt, bitCapInt, const cplx<R>*, bool, hipStream_t);                                   \
    template void launchQftColumnGeneral<R>(                                                        \
        cplx<R>*, bitCapInt, bitCapInt, const RampArgs&, double, bool, hipStream_t);

QA_INSTANTIATE(float)
QA_INSTANTIATE(double)

// ---- dense k-qubit gate: one tiled pass -------------------------------------
// Defined and instantiated after the list above, so that the kernels of that
// list keep their order in the code object.

__device__ __forceinline__ float mtrxnFma1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double mtrxnFma1(double a, double b, double c) { return __builtin_fma(a, b, c); }

// acc += m * x as four fused multiply-adds
template <typename R> __device__ __forceinline__ void mtrxnFma(cplx<R>& acc, cplx<R> m, cplx<R> x)
{
    acc.re = mtrxnFma1(m.re, x.re, acc.re);
    acc.im = mtrxnFma1(m.re, x.im, acc.im);
    acc.re = mtrxnFma1(-m.im, x.im, acc.re);
    acc.im = mtrxnFma1(m.im, x.re, acc.im);
}

// RPT output rows of one orbit: the orbit's 2^K inputs stream from LDS once
// for all of them. UNI: the row block is the same for the whole wave (the tile
// holds at least 64 orbits), so the matrix entries are scalar loads; two
// columns a trip keep them within the scalar registers. Otherwise they are
// vector loads, one column a trip.
template <typename R, int K, int RPT, bool UNI>
__device__ __forceinline__ void mtrxnRows(const cplx<R>* tile, const cplx<R>* __restrict__ dm,
    int oBits, unsigned o, unsigned rb, cplx<R>* acc)
{
    constexpr int D = 1 << K;
    constexpr int CU = UNI ? 2 : 1;
    if constexpr (UNI) rb = (unsigned)__builtin_amdgcn_readfirstlane((int)rb);
    const cplx<R>* __restrict__ rows = dm + (size_t)rb * RPT * D;
#pragma unroll
    for (int i = 0; i < RPT; ++i) acc[i] = cplx<R>(0, 0);
#pragma unroll 1
    for (int c0 = 0; c0 < D; c0 += CU) {
        cplx<R> x[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) x[u] = tile[mtrxnSlot(K, oBits, (unsigned)(c0 + u), o)];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
#pragma unroll
            for (int u = 0; u < CU; ++u) mtrxnFma(acc[i], rows[i * D + c0 + u], x[u]);
        }
    }
}

// A workgroup strides over its tiles (mtrxn_plan.hpp): stage the tile with
// 16-byte global accesses, mat-vec every orbit that passes the in-tile
// controls, store the tile back. With up to 2^(TB-8) rows a thread owns whole
// orbits and works in registers; above, 2^K / RPT threads share an orbit, keep
// their accumulators across a barrier and write them to the slots they read.
// A smaller state leaves threads idle in the same code.
template <typename R, int K>
__global__ __launch_bounds__(QA_MTRXN_BLOCK) void k_mtrx_n(
    cplx<R>* __restrict__ sv, const cplx<R>* __restrict__ dm, const MtrxNArgs<R> a)
{
    constexpr int TB = qaLdsTileBits<R>();
    constexpr int D = 1 << K;
    constexpr int RPT = mtrxnRowsPerThread(K, TB);
    constexpr int G = D / RPT;
    constexpr unsigned VEC = sizeof(R) == 4 ? 2 : 1; // amplitudes per 16-byte access
    constexpr unsigned STEP = QA_MTRXN_BLOCK * VEC;
    static_assert(G == 1 || G * (1 << (TB - K)) <= QA_MTRXN_BLOCK, "one work item per thread");
    __shared__ cplx<R> tile[1u << TB];
    const MtrxNGeom& g = a.g;
    const unsigned tileLen = 1u << g.m;
    const int oBits = g.m - K;
    const unsigned nOrb = 1u << oBits;
    const unsigned tid = threadIdx.x;
    // the staging maps are linear over XOR: thread part here, trip part (wave
    // uniform) in the loop
    const unsigned lLo = tid * VEC;
    const unsigned slotLo = mtrxnLdsAddr(g, lLo);
    const bitCapInt offLo = mtrxnGlobalOff(g, lLo);
    const unsigned slot1 = mtrxnLdsAddr(g, 1u);
    const cplx<R>* __restrict__ mp = K <= 3 ? a.m : dm;

    for (bitCapInt t = blockIdx.x; t < g.nTiles; t += gridDim.x) {
        cplx<R>* base = sv + mtrxnTileBase(g, t);
        for (unsigned lHi = 0; lHi < tileLen; lHi += STEP) {
            if ((lHi | lLo) >= tileLen) continue;
            const unsigned s = slotLo ^ mtrxnLdsAddr(g, lHi);
            const bitCapInt off = offLo | mtrxnGlobalOff(g, lHi);
            if constexpr (VEC == 2) {
                const float4 v = *reinterpret_cast<const float4*>(base + off);
                tile[s] = cplx<R>(v.x, v.y);
                tile[s ^ slot1] = cplx<R>(v.z, v.w);
            } else {
                tile[s] = base[off];
            }
        }
        __syncthreads();

        if constexpr (G == 1) {
            for (unsigned o = tid; o < nOrb; o += QA_MTRXN_BLOCK) {
                if ((o & g.cMaskO) != g.cValO) continue;
                cplx<R> v[D];
#pragma unroll
                for (int c = 0; c < D; ++c) v[c] = tile[mtrxnSlot(K, oBits, (unsigned)c, o)];
                // rows stay a loop from 8 x 8 on: unrolled, the whole matrix
                // is hoisted into scalar registers and spills
#pragma unroll(D >= 8 ? 2 : D)
                for (int r = 0; r < D; ++r) {
                    cplx<R> acc(0, 0);
#pragma unroll
                    for (int c = 0; c < D; ++c) mtrxnFma(acc, mp[r * D + c], v[c]);
                    tile[mtrxnSlot(K, oBits, (unsigned)r, o)] = acc;
                }
            }
            __syncthreads();
        } else {
            const unsigned o = tid & (nOrb - 1u);
            const unsigned rb = tid >> oBits;
            const bool active = rb < (unsigned)G && (o & g.cMaskO) == g.cValO;
            cplx<R> acc[RPT];
            if (active) {
                if (nOrb >= 64u) {
                    mtrxnRows<R, K, RPT, true>(tile, mp, oBits, o, rb, acc);
                } else {
                    mtrxnRows<R, K, RPT, false>(tile, mp, oBits, o, rb, acc);
                }
            }
            __syncthreads();
            if (active) {
#pragma unroll
                for (int i = 0; i < RPT; ++i) {
                    tile[mtrxnSlot(K, oBits, rb * RPT + (unsigned)i, o)] = acc[i];
                }
            }
            __syncthreads();
        }

        for (unsigned lHi = 0; lHi < tileLen; lHi += STEP) {
            if ((lHi | lLo) >= tileLen) continue;
            const unsigned s = slotLo ^ mtrxnLdsAddr(g, lHi);
            const bitCapInt off = offLo | mtrxnGlobalOff(g, lHi);
            if constexpr (VEC == 2) {
                const cplx<R> x = tile[s], y = tile[s ^ slot1];
                *reinterpret_cast<float4*>(base + off) = make_float4(x.re, x.im, y.re, y.im);
            } else {
                base[off] = tile[s];
            }
        }
        __syncthreads();
    }
}

template <typename R, int K>
static void launchMtrxNK(cplx<R>* sv, const cplx<R>* dm, const MtrxNArgs<R>& a, hipStream_t stream)
{
    const int grid = ldsGridFor(a.g.nTiles);
    hipLaunchKernelGGL(
        (k_mtrx_n<R, K>), dim3(grid), dim3(QA_MTRXN_BLOCK), 0, stream, sv, dm, a);
}

template <typename R>
void launchMtrxN(cplx<R>* sv, const cplx<R>* dm, const MtrxNArgs<R>& a, hipStream_t stream)
{
    switch (a.g.k) {
    case 1: launchMtrxNK<R, 1>(sv, dm, a, stream); break;
    case 2: launchMtrxNK<R, 2>(sv, dm, a, stream); break;
    case 3: launchMtrxNK<R, 3>(sv, dm, a, stream); break;
    case 4: launchMtrxNK<R, 4>(sv, dm, a, stream); break;
    case 5: launchMtrxNK<R, 5>(sv, dm, a, stream); break;
    default: launchMtrxNK<R, 6>(sv, dm, a, stream); break;
    }
}

template void launchMtrxN<float>(cplx<float>*, const cplx<float>*, const MtrxNArgs<float>&, hipStream_t);
template void launchMtrxN<double>(
    cplx<double>*, const cplx<double>*, const MtrxNArgs<double>&, hipStream_t);

} // namespace qrack_amd
