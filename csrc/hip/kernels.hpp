// qrack_amd — HIP kernel launch API (host-visible declarations).
//
// Capability parity target: the reference GPU kernel inventory
// (/root/reference/src/common/qengine.cl 74 kernels + qheader_alu.cl;
// SURVEY.md §2.2). Fresh CDNA4 design: wave64 blocks of 256, grid-stride
// loops capped near 8 blocks/CU (256 CUs), float4/double2-vectorized
// amplitude streaming, single-pass two-stage reductions (wave shuffle +
// LDS + per-block partials), and one uniform-opcode permutation kernel for
// the whole ALU family instead of 26 near-identical kernels.
#pragma once

#include "../common/types.hpp"
#include "../krylov.hpp"
#include "mtrxn_plan.hpp"
#include "rdm_plan.hpp"

#include <hip/hip_runtime.h>

namespace qrack_amd {

constexpr int QA_MAX_SKIP_POWERS = 16;
// grid-size cap for gate/reduction launches; partials buffers must hold
// this many (A/B-swept on the 30q QFT: 32768 = 104.4 ms < 16384 = 106.1 <
// 8192 = 108.0 < 2048 = 112.1 — more blocks shrink the grid-stride tails
// and balance the 8 XCDs)
constexpr int QA_REDUCE_MAX_BLOCKS = 32768;

// by-value argument block for gate kernels
template <typename R> struct GateArgs {
    cplx<R> m[4];
    bitCapInt offset1;
    bitCapInt offset2;
    bitCapInt qPowers[QA_MAX_SKIP_POWERS]; // sorted ascending
    int nPowers;
    bitCapInt maxI; // iterations (pairs)
};

enum class PermOp : int {
    INC = 0,
    INCDECC,
    INCS,
    MUL,
    DIV,
    MULMODN,
    IMULMODN,
    POWMODN,
    HASH,
    LDA,
    ADC,
    SBC,
    ROL,
    INCBCD,
};

struct PermArgs {
    int op;
    bitCapInt maxI;                        // iterated indices (sub-space size)
    bitCapInt qPowers[QA_MAX_SKIP_POWERS]; // skip powers for the iteration
    int nPowers;
    bitCapInt controlMask; // OR into every iterated index
    bitLenInt start;       // in/out register start
    bitLenInt length;      // register length
    bitCapInt operand;     // toAdd / toMul / base
    bitCapInt modN;
    bitCapInt carryMask;    // carry / overflow qubit power
    bitLenInt start2;       // out register start (modN ops) / value start (LDA)
    bitLenInt length2;      // out register length
    bitCapInt extra;        // carry-in addend etc.
    const unsigned char* table; // device pointer for HASH/LDA/ADC/SBC
    int tableBytes;             // bytes per table entry
};

enum class ReduceOp : int {
    NORM_ALL = 0,   // sum |amp|^2
    PROB_BITSET,    // sum |amp|^2 where (i & mask) == mask (single-bit use)
    PROB_MASK,      // sum |amp|^2 where (i & mask) == perm
    PROB_PARITY,    // sum |amp|^2 where parity(i & mask)
    EXP_PERM,       // sum value(i) * |amp|^2 (factorized bit values)
    EXP_PERM_SQ,    // sum value(i)^2 * |amp|^2
    NORM_FLOOR,     // sum |amp|^2 with amplitude floor (UpdateRunningNorm)
};

constexpr int QA_REDUCE_MAX_BITS = 32;

struct ReduceArgs {
    bitCapInt maxI;
    bitCapInt mask;
    bitCapInt perm;
    double offset;       // EXP_PERM value offset
    double normThresh;   // NORM_FLOOR
    // EXP_PERM inputs ride IN the kernarg segment (<= 32 listed bits; the
    // engine falls back to the generic host path beyond that) — no device
    // staging buffers, so no stream-ordered-allocator exposure on the
    // expectation/variance query path
    bitLenInt bitsArr[QA_REDUCE_MAX_BITS];
    bitCapInt permsArr[QA_REDUCE_MAX_BITS];
    int nBits;
};

// One launch of the Pauli-sum pass: up to QA_PAULI_MAX_TERMS strings that
// share the flip mask x, each with its sign mask z and weight coeff * i^ny.
// Terms [0, nRe) carry real weights, [nRe, nTerms) imaginary ones. Like
// ReduceArgs the table rides in the kernarg segment (~530 B), so the per-term
// loop reads it with scalar loads and no staging buffer exists.
constexpr int QA_PAULI_MAX_TERMS = 32;

struct PauliArgs {
    bitCapInt x;     // X/Y mask; 0 selects the diagonal kernel
    bitCapInt nAmps; // 2^qubits
    int nRe;
    int nTerms;
    bitCapInt z[QA_PAULI_MAX_TERMS];
    double w[QA_PAULI_MAX_TERMS];
};

// One launch of the in-place Pauli-evolution pass on the pairs (i, i^x): up to
// QA_PAULI_EVOLVE_MAX_SEGS segments, each a run of terms of one parity set
// (entries [segEnd[k-1], segEnd[k]) of z / w). w holds tau * weight, formed
// in double on the host, so a pair's rotation angle in a segment is the signed
// sum of that segment's w. A launch whose segments all hold ONE term takes the
// transcendental-free kernel: |angle| is constant, the host leaves
// cos / sin of w[k] in segCos / segSin and the kernel only picks sin's sign
// from the parity. phase (when hasPhase) is a scalar every amplitude is
// multiplied by last. Like PauliArgs the table rides in the kernarg segment.
constexpr int QA_PAULI_EVOLVE_MAX_SEGS = 4;

struct PauliEvolveArgs {
    bitCapInt x;     // X/Y mask; 0 selects the diagonal kernel (one re segment)
    bitCapInt nAmps; // 2^qubits
    int nSeg;
    int hasPhase;
    int segEnd[QA_PAULI_EVOLVE_MAX_SEGS];
    int segIm[QA_PAULI_EVOLVE_MAX_SEGS]; // 0: re-set rotation, 1: im-set rotation
    double segCos[QA_PAULI_EVOLVE_MAX_SEGS];
    double segSin[QA_PAULI_EVOLVE_MAX_SEGS];
    double phaseRe, phaseIm;
    bitCapInt z[QA_PAULI_MAX_TERMS];
    double w[QA_PAULI_MAX_TERMS];
};

// One fused step of the adjoint-gradient sweep for the rotation
// exp(-i theta P) of ONE string P = i^ny (-1)^popcount(i&z) |i^x><i|: the
// launch sums <lam|P|psi> and applies exp(+i theta P) to both vectors. w is
// the real factor of i^ny (+1 or -1) and im says whether a factor i remains;
// cs / sn are the host's cos / sin of -theta * w, as segCos / segSin are.
struct PauliAdjointArgs {
    bitCapInt x;     // X/Y mask; 0 selects the diagonal kernel
    bitCapInt z;
    bitCapInt nAmps; // 2^qubits
    int im;
    double w;
    double cs, sn;
};

// reduced density matrix, register regime (rdm_plan.hpp): kept powers
// ascending, and the state offset of every kept index in that order
struct RdmRegArgs {
    bitCapInt pows[QA_RDM_REG_MAX];
    bitCapInt off[1 << QA_RDM_REG_MAX];
    bitCapInt nItems; // environment rows; row pairs in fp32 with qubit 0 not kept
};

// ... tile regime: one launch of the plan
struct RdmTileArgs {
    bitCapInt tileMask;     // state bits that address the tile: kept-in-tile + low environment
    bitCapInt tileMaskHigh; // tileMask without the bits a block covers in one trip
    bitCapInt enumMask;     // environment bits that number the tiles
    bitCapInt rowOff;       // block bits at the row-side value
    bitCapInt colOff;       // ... at the column-side value
    bitCapInt nTiles;
    uint32_t keptInTile;    // the kept bits, as a mask over the tile's own index
    int tileAddrBits;       // T: a tile holds 2^T amplitudes
    int cross;              // rowOff != colOff: two tiles
};

// ---- launches (all asynchronous on `stream`) -------------------------------

// Reduced density matrix passes. Stage 1 leaves one set of double partials
// per block in partialsDev (rdmRegGrid / rdmTileGrid sets of 4^k or
// 32 * rdmTilePatches doubles), stage 2 folds them in a fixed order into
// resultDev. Read sv only.
int rdmRegGrid(bitCapInt nItems);
int rdmTileGrid(bitCapInt nTiles);
template <typename R>
void launchRdmReg(const cplx<R>* sv, int k, bool keepsBit0, const RdmRegArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream);
template <typename R>
void launchRdmTile(const cplx<R>* sv, int kt, const RdmTileArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream);


// One read-and-write pass: every amplitude is loaded once and stored once, by
// exactly one thread.
template <typename R>
void launchPauliEvolve(cplx<R>* sv, const PauliEvolveArgs& a, hipStream_t stream);

// sum_t w_t <psi|P_t|psi> for one group: stage 1 leaves per-block partials in
// partialsDev (QA_REDUCE_MAX_BLOCKS doubles), stage 2 folds them in a fixed
// order into *resultDev. Reads sv only.
template <typename R>
void launchPauliGroup(const cplx<R>* sv, const PauliArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream);

// Every pair-walk launch that reduces (launchPauliGroup above, the launches
// below and launchKrylovApply) uses the reduction grid, capped by
// QRACK_GPU_BLOCKS when that is set; launchPauliApply uses the same grid and
// launchPauliEvolve the exact streaming grid under the same cap. For the
// complex results of launchPauliBraket and launchPauliAdjoint partialsDev
// holds 2 * QA_REDUCE_MAX_BLOCKS doubles (real parts, then imaginary parts)
// and resultDev takes (re, im).

// <bra| ident + sum_t w_t P_t |psi> for one group; reads both vectors only
template <typename R>
void launchPauliBraket(const cplx<R>* psi, const cplx<R>* bra, const PauliArgs& a, double ident,
    double* partialsDev, double* resultDev, hipStream_t stream);

// dest = (ident + sum_t w_t P_t) psi when `first` (dest is not read), else
// dest += (sum_t w_t P_t) psi. dest must not alias psi.
template <typename R>
void launchPauliApply(const cplx<R>* psi, cplx<R>* dest, const PauliArgs& a, double ident, bool first,
    hipStream_t stream);

// resultDev <- <lam|P|psi>, then psi and lam <- exp(+i theta P) of themselves
template <typename R>
void launchPauliAdjoint(cplx<R>* psi, cplx<R>* lam, const PauliAdjointArgs& a, double* partialsDev,
    double* resultDev, hipStream_t stream);

// One fused Lanczos step on the unnormalised basis (krylov.hpp): L apply
// launches, then one finish. The weights of `a`, ident and bcoef arrive scaled
// by the host. All three use the reduction grid under the QRACK_GPU_BLOCKS cap.
//
// dest = (ident + sum_t w_t P_t) u - bcoef prev when `first` (dest is not read;
// prev may be null: no such term), else dest += (sum_t w_t P_t) u. *slotDev
// takes the launch's share of Re <u|dest>, block partials (QA_REDUCE_MAX_BLOCKS
// doubles in partialsDev) folded on the device. dest aliases neither input.
template <typename R>
void launchKrylovApply(const cplx<R>* u, const cplx<R>* prev, cplx<R>* dest, const PauliArgs& a, double ident,
    double bcoef, bool first, double* partialsDev, double* slotDev, hipStream_t stream);

// w <- w - a u with a = scale * (slotsDev[0] + ... + slotsDev[nSlots - 1]),
// read on the device; resultDev <- (sum of the slots, ||w||^2). With !store w
// is left as it was and only the norm is formed.
template <typename R>
void launchKrylovFinish(const cplx<R>* u, cplx<R>* w, bitCapInt nAmps, const double* slotsDev, int nSlots,
    double scale, bool store, double* partialsDev, double* resultDev, hipStream_t stream);

// state <- coef[0] state + sum_j coef[j + 1] src[j], complex coefficients
// formed in double by the host, for up to KRYLOV_COMBINE_MAX_VECTORS sources
template <typename R> struct KrylovCombineArgs {
    const cplx<R>* src[KRYLOV_COMBINE_MAX_VECTORS];
    double coefRe[KRYLOV_COMBINE_MAX_VECTORS + 1];
    double coefIm[KRYLOV_COMBINE_MAX_VECTORS + 1];
    int nSrc;
};

template <typename R>
void launchKrylovCombine(cplx<R>* state, bitCapInt nAmps, const KrylovCombineArgs<R>& a, hipStream_t stream);

// Orthogonalisation of LanczosLowestStates (krylov.hpp) against one chunk of
// n <= KRYLOV_ORTH_MAX_VECTORS unnormalised basis vectors. With coefDev:
// w <- w - sum_i (scale[i] * (coefDev[2i] + i coefDev[2i + 1])) u[i] first
// (stored only with `store`). Then resultDev[2i], resultDev[2i + 1] <- (re, im)
// of <u[i]|w> and resultDev[32] <- ||w||^2, of that w. coefDev is the
// resultDev of an earlier launch on the stream, or null: the read-only
// inner-product pass. partialsDev holds KRYLOV_ORTH_RESULTS *
// krylovOrthGrid(items) doubles, items = nAmps (fp64) or nAmps / 2 (fp32);
// the grid obeys the QRACK_GPU_BLOCKS cap.
constexpr int KRYLOV_ORTH_RESULTS = 2 * KRYLOV_ORTH_MAX_VECTORS + 1;
// Two blocks per CU are resident whatever the register count turns out to be,
// and 17 loads of 16 B in flight per thread keep HBM busy from there; the cap
// also lets the partials fit the engine's reduction buffer.
constexpr int KRYLOV_ORTH_MAX_BLOCKS = 512;
static_assert(KRYLOV_ORTH_RESULTS * KRYLOV_ORTH_MAX_BLOCKS <= 2 * QA_REDUCE_MAX_BLOCKS,
    "the orth partials live in the reduction partials buffer");
template <typename R> struct KrylovOrthArgs {
    const cplx<R>* u[KRYLOV_ORTH_MAX_VECTORS];
    double scale[KRYLOV_ORTH_MAX_VECTORS];
    int n;
};
int krylovOrthGrid(bitCapInt nItems);
template <typename R>
void launchKrylovOrth(cplx<R>* w, bitCapInt nAmps, const KrylovOrthArgs<R>& a, const double* coefDev,
    bool store, double* partialsDev, double* resultDev, hipStream_t stream);

// The restart's rotation: out[i] <- sum_r mDev[r * 16 + i] in[r], i < kp,
// r < k, a real matrix in R with rows padded to KRYLOV_COMBINE_MAX_VECTORS.
// Elementwise across the buffers: an out[i] may be one of the in[r].
template <typename R> struct KrylovRotateArgs {
    const cplx<R>* in[KRYLOV_MAX_DIM];
    cplx<R>* out[KRYLOV_COMBINE_MAX_VECTORS];
    int k, kp;
};
template <typename R>
void launchKrylovRotate(const KrylovRotateArgs<R>& a, const R* mDev, bitCapInt nAmps, hipStream_t stream);

template <typename R>
void launchApply2x2(cplx<R>* sv, const GateArgs<R>& a, hipStream_t stream);

template <typename R>
void launchUniformlyControlled(cplx<R>* sv, bitCapInt maxI, bitCapInt targetPower,
    const bitCapInt* ctrlPowersDev, int nCtrls, const cplx<R>* mtrxsDev, hipStream_t stream);

template <typename R>
void launchXMask(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, hipStream_t stream);

template <typename R>
void launchParityPhase(
    cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, cplx<R> even, cplx<R> odd, hipStream_t stream);

// two-stage reduction: stage 1 fills partials[gridSize]; returns grid size used
template <typename R>
int launchReduce(const cplx<R>* sv, const ReduceArgs& a, int op, double* partialsDev,
    hipStream_t stream);

// argmax of |amp|^2: fills (value,index) pairs per block
template <typename R>
int launchArgMax(const cplx<R>* sv, bitCapInt maxI, double* valsDev, bitCapInt* idxDev,
    hipStream_t stream);

template <typename R>
void launchNormalize(
    cplx<R>* sv, bitCapInt maxQPower, cplx<R> factor, R normThresh, hipStream_t stream);

template <typename R>
void launchApplyM(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, bitCapInt result, cplx<R> nrm,
    hipStream_t stream);

template <typename R>
void launchApplyParity(cplx<R>* sv, bitCapInt maxQPower, bitCapInt mask, bool odd, cplx<R> nrm,
    hipStream_t stream);

template <typename R>
void launchCompose(const cplx<R>* a, const cplx<R>* b, cplx<R>* out, bitCapInt nMaxQPower,
    bitLenInt start, bitLenInt oQubits, hipStream_t stream);

// out[r] = in[low | (slicePerm << start) | high] * scale  (Dispose/Decompose)
template <typename R>
void launchDisposeSlice(const cplx<R>* in, cplx<R>* out, bitCapInt remPower, bitLenInt start,
    bitLenInt length, bitCapInt slicePerm, cplx<R> scale, hipStream_t stream);

// dest[p] = in[low(rem) | (p << start) | high(rem)] * scale  (Decompose part)
template <typename R>
void launchGatherPart(const cplx<R>* in, cplx<R>* dest, bitCapInt partPower, bitLenInt start,
    bitLenInt length, bitCapInt remIndex, cplx<R> scale, hipStream_t stream);

// out[i] = (mid(i)==0) ? in[collapse(i)] : 0   (Allocate)
template <typename R>
void launchAllocateExpand(const cplx<R>* in, cplx<R>* out, bitCapInt nMaxQPower, bitLenInt start,
    bitLenInt length, hipStream_t stream);

// swap upper half of a with lower half of b
template <typename R>
void launchShuffleSwap(cplx<R>* aHigh, cplx<R>* bLow, bitCapInt half, hipStream_t stream);

template <typename R>
void launchPermute(const cplx<R>* sv, cplx<R>* nsv, const PermArgs& a, hipStream_t stream);

// nsv[i] = ((i & controlMask) == controlMask) ? 0 : sv[i]
template <typename R>
void launchCopyUncontrolled(
    const cplx<R>* sv, cplx<R>* nsv, bitCapInt maxQPower, bitCapInt controlMask, hipStream_t stream);

template <typename R>
void launchPhaseFlipIfLess(cplx<R>* sv, bitCapInt maxQPower, bitCapInt greaterPerm, bitLenInt start,
    bitCapInt regMask, bitCapInt flagMask, hipStream_t stream);

int reduceGridSize(bitCapInt n);

// fused diagonal phase ramp: amp *= exp(i*scale*((x>>rampStart) mod
// 2^rampBits)) where (condPower==0) || (x & condPower) — one pass replaces
// rampBits (controlled-)phase gates (the QFT column ladder).
template <typename R>
void launchPhaseRamp(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt rampBits,
    bitCapInt condPower, double scale, hipStream_t stream);

// generalized diagonal ramp with relocated bits: frac(i) =
// ((i >> rampStart) & inPlaceRelMask) + sum_k (i & sPow[k] ? sWeight[k] : 0);
// amp *= exp(i*scale*frac) where (condPow==0)||(i & condPow). Supports the
// distributed pager's lazily-permuted qubit maps (<= 8 relocated bits).
struct RampArgs {
    bitLenInt rampStart;
    bitCapInt inPlaceRelMask;
    int nScattered;
    bitCapInt sPow[8];
    uint64_t sWeight[8];
    bitCapInt condPow;
    double scale;
};

template <typename R>
void launchPhaseRampGeneral(cplx<R>* sv, bitCapInt maxQPower, const RampArgs& a, hipStream_t stream);

// TWO fused QFT columns in one state pass (see kernels.hip k_qft_col2):
// columns (col, col-1) as 4-amplitude orbits — ONE sincos per orbit drives
// both ramps (cross term is a constant ±i factor, lower ramp = f0^2)
template <typename R>
void launchQftColumn2(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tHi, bitCapInt tLo, int sign, bool pre, hipStream_t stream);

// ladder group width: uniform K=4 fp32 / K=3 fp64 — the engine must align
// low-ladder lengths to a multiple of this
template <typename R> constexpr int qaLowLadderK() { return sizeof(R) == 4 ? 4 : 3; }

// one-pass low-bit QFT ladder: columns colMax..0 applied inside contiguous
// 2^tb-amplitude LDS tiles (start-0 registers only; colMax+1 must be a
// multiple of qaLowLadderK<R>())
template <typename R>
void launchQftLowLds(
    cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, int sign, bool pre, hipStream_t stream);

// nCols mid-range QFT columns per pass through a 2D LDS tile (64 contiguous
// low amps x 2^nCols column-bit combos; start-0 registers, colLo >= 6).
// nCols in {2, 3, 4, 6}: 32 KB of LDS at 6 columns fp32. More columns per
// pass go through launchQftMidWide; the planner in qft_plan.hpp chooses.
template <typename R>
void launchQftMidLds(cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, int sign, bool pre,
    hipStream_t stream);

// "source is a basis state" variants of the two LDS passes: the buffer's
// contents are undefined and the first gather is synthesised as
// index == perm ? phase : 0 — a write-only pass whose stores are
// bit-identical to the normal kernel run on the materialised basis state
template <typename R>
void launchQftLowLdsBasis(cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, int sign, bool pre,
    bitCapInt perm, cplx<R> phase, hipStream_t stream);

template <typename R>
void launchQftMidLdsBasis(cplx<R>* sv, bitCapInt maxQPower, int colLo, int nCols, int sign,
    bool pre, bitCapInt perm, cplx<R> phase, hipStream_t stream);

// Wide-tile mid pass, fp32 only: nCols = 9 (three K=3 orbit groups) or 8
// (two K=4 groups) columns colLo..colLo+nCols-1 through a 2D LDS tile of
// 2^lowBits contiguous low amplitudes x 2^nCols column-bit combinations.
// lowBits = 4: 128-byte runs, 64 KB (9 columns, 512 threads) or 32 KB (8
// columns, 256 threads) of LDS per block; lowBits = 5: 256-byte runs,
// 128 KB / 64 KB, 1024 / 512 threads. Tiles of 64 KB and more have the
// kernel's dynamic-LDS limit raised on first use. Requires a start-0
// register, colLo >= lowBits and maxQPower >= 2^(colLo+nCols). basis: the
// source is phase·|perm> and the buffer is undefined, as in
// launchQftMidLdsBasis (write-only, stores bit-identical to basis = false
// run on the materialised state); perm and phase are ignored otherwise.
void launchQftMidWide(cplx<float>* sv, bitCapInt maxQPower, int lowBits, int colLo, int nCols,
    int sign, bool pre, bool basis, bitCapInt perm, cplx<float> phase, hipStream_t stream);

// Support-restricted passes of a transform of the basis state phase·|perm>
// (schedule: qftSupportPlan in qft_plan.hpp), fp32 only. The input of the
// pass can be nonzero only where ((x ^ perm) & fixedMask) == 0; there it is
// `phase` (fromBuffer = 0) or sv[x] (fromBuffer != 0), everywhere else +0 and
// the buffer is NOT read: outside the support it holds nothing defined. The
// pass visits the activeTiles tiles whose index is tileFixed with the bits of
// tileFree counted through, and writes each of them whole; the stores are
// bit-identical to the normal kernel's on the materialised state wherever
// that state is nonzero.
struct QftSupportArgs {
    bitCapInt perm;
    bitCapInt fixedMask;
    bitCapInt tileFree;
    bitCapInt tileFixed;
    bitCapInt activeTiles; // 2^popcount(tileFree)
    int fromBuffer;
};

// low ladder; tileSumsDev != nullptr (forward only, all tiles active) also
// leaves the per-tile norms as launchQftLowLdsSums does
void launchQftLowLdsSupport(cplx<float>* sv, bitCapInt maxQPower, int tb, int colMax, int sign,
    bool pre, const QftSupportArgs& sup, cplx<float> phase, double* tileSumsDev,
    hipStream_t stream);

// Forward last low pass of a support plan over 8 or 12 columns, running only
// the 16-point orbits that hold a nonzero input (qftSparseLastPlan in
// qft_plan.hpp, taken from sup.perm): one, sixteen and 256 per tile instead
// of 256 in every group. The other orbits transform +0 inputs under twiddles
// that depend on the position alone, so their outputs are one pattern of
// signed zeros for every tile: launchQftSparseZeroTemplate leaves it in
// zeroTplDev (two sign bits per in-tile index and group,
// QA_QFT_ZERO_TPL_BYTES bytes), and an orbit with a nonzero input takes its
// fifteen partners from there. The stores and tile sums are bit-identical to
// launchQftLowLdsSupport's. zeroTplDev must hold the template of the same
// nCols. A block takes four consecutive active tiles at a time: the groups
// at gLo = 8 and gLo = 4 run for the whole batch at once, the group at
// gLo = 0 and the write-out tile by tile with each wave on its own quarter
// (kernels.hip). One block per batch up to the usual cap; QRACK_GPU_BLOCKS
// caps the grid further, the blocks then stride over the batches.
constexpr size_t QA_QFT_ZERO_TPL_BYTES = 2u << 12;
void launchQftSparseZeroTemplate(unsigned char* zeroTplDev, int nCols, hipStream_t stream);
void launchQftLowSparseLast(cplx<float>* sv, bitCapInt maxQPower, int tb, int colMax,
    const QftSupportArgs& sup, cplx<float> phase, const unsigned char* zeroTplDev,
    double* tileSumsDev, hipStream_t stream);

// mid pass: nCols in {2, 3, 4, 6} on the 64-wide tile, 8 or 9 on the wide
// one with 2^lowBits-amplitude runs (as launchQftMidLds / launchQftMidWide)
void launchQftMidSupport(cplx<float>* sv, bitCapInt maxQPower, int lowBits, int colLo, int nCols,
    int sign, bool pre, const QftSupportArgs& sup, cplx<float> phase, hipStream_t stream);

// forward low ladder that also writes tileSumsDev[t] = sum |amp|^2 of the
// 2^tb amplitudes it stored for tile t (maxQPower >> tb doubles; fixed
// reduction order, no atomics)
template <typename R>
void launchQftLowLdsSums(cplx<R>* sv, bitCapInt maxQPower, int tb, int colMax, double* tileSumsDev,
    hipStream_t stream);

// sums[c] = tileSums[c*tilesPerChunk .. (c+1)*tilesPerChunk) added in a
// fixed order — replaces launchChunkSums when tile sums are valid
void launchTileChunkSums(const double* tileSumsDev, bitCapInt nChunks, bitCapInt tilesPerChunk,
    double* sumsDev, hipStream_t stream);

// sv[perm] = amp from a one-thread kernel (no host staging, no sync)
template <typename R>
void launchSetAmp(cplx<R>* sv, bitCapInt perm, cplx<R> amp, hipStream_t stream);

// generic K-column fused QFT pass (2^K-amplitude orbits; K=4 instantiated)
template <typename R>
void launchQftColumnK(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    int kCols, const bitCapInt* tPows, int sign, bool pre, hipStream_t stream);

// THREE fused QFT columns per pass (8-amplitude orbits; see k_qft_col3)
template <typename R>
void launchQftColumn3(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tHi, bitCapInt tMid, bitCapInt tLo, int sign, bool pre, hipStream_t stream);

// generalized fused QFT column: H on tPow + the (possibly relocated-bit)
// ramp of RampArgs in ONE pass; phase0 is a constant phase folded onto the
// target=1 side (distributed pager meta-page scalar)
template <typename R>
void launchQftColumnGeneral(cplx<R>* sv, bitCapInt maxQPower, bitCapInt tPow, const RampArgs& a,
    double phase0, bool pre, hipStream_t stream);

// TWO generalized columns per pass (arbitrary local target slots,
// relocated ramp bits, per-column meta scalars) — the distributed pager's
// local-ladder pass-halving (see k_qft_col2_gen)
template <typename R>
void launchQftColumn2General(cplx<R>* sv, bitCapInt maxQPower, bitCapInt tPowHi, bitCapInt tPowLo,
    const RampArgs& a, double phase0Hi, double phase0Lo, bool pre, hipStream_t stream);

// Ranged top-target fused QFT column for the distributed pager's PIPELINED
// page exchange: processes pair rows r in [itLo, itHi) of the H on the TOP
// local qubit (tPow = maxQPower/2), reading ONE side of each pair straight
// from the RCCL receive buffer `recvSrc` (indexed r - itLo) instead of the
// state vector — the received chunk is consumed in place, no staging copy.
// recvIsLow: true when the received chunk is the pair's low (target=0) side
// (the HIGH page of an exchange receives the low side). Launched per chunk
// on the caller-supplied stream (torch's current stream) so NCCL chunk c+1
// overlaps with chunk c's compute. Replaces the host-staged ShuffleBuffers
// swap of the reference (opencl.cpp:254-264) with exchange+apply fusion.
template <typename R>
void launchQftColumnTopRange(cplx<R>* sv, bitCapInt maxQPower, const RampArgs& a, double phase0,
    bool pre, bitCapInt itLo, bitCapInt itHi, const cplx<R>* recvSrc, bool recvIsLow,
    hipStream_t stream);

// batched independent single-qubit gates: k distinct-target 2x2s applied in
// ONE full-state pass (2^k-amplitude orbits in registers). The memory-bound
// fusion win: k passes -> 1. fp32 supports k in [2,5], fp64 [2,4].
constexpr int QA_MAX_BATCH_1Q = 5;

template <typename R> struct Batch1qArgs {
    cplx<R> m[4 * QA_MAX_BATCH_1Q];
    bitCapInt tPow[QA_MAX_BATCH_1Q]; // sorted ascending, distinct
    int k;
    bitCapInt maxI; // orbit count = maxQPower >> k
};

template <typename R>
void launchMtrx1qBatch(cplx<R>* sv, const Batch1qArgs<R>& a, hipStream_t stream);

// LDS-tiled low-bit batch: gates whose targets all sit below QA_LDS_TILE_BITS
// apply inside a shared-memory tile — up to 12 gates in ONE global RMW pass
// (the register-orbit kernels degrade on low-bit targets; LDS does not).
// 32 KB LDS tiles both ways: 4096 fp32 amps / 2048 fp64 amps (a 64 KB fp64
// tile would sit exactly on the per-workgroup LDS limit)
template <typename R> constexpr int qaLdsTileBits() { return sizeof(R) == 4 ? 12 : 11; }
// register-orbit group width inside the LDS gate-batch kernel; the engine
// pads batches to a multiple of this with identity gates
template <typename R> constexpr int qaLdsBatchK() { return sizeof(R) == 4 ? 4 : 3; }
constexpr int QA_LDS_TILE_BITS = 12; // fp32 value; use qaLdsTileBits<R>()
constexpr int QA_MAX_BATCH_LDS = 12;

template <typename R> struct BatchLdsArgs {
    cplx<R> m[4 * QA_MAX_BATCH_LDS];
    bitCapInt tPow[QA_MAX_BATCH_LDS]; // sorted ascending, all < 2^QA_LDS_TILE_BITS
    int k;
    bitCapInt maxQPower;
};

template <typename R>
void launchMtrx1qBatchLds(cplx<R>* sv, const BatchLdsArgs<R>& a, hipStream_t stream);

// LDS-tiled batch of disjoint TWO-qubit 4x4 gates (all four qubit bits below
// the tile): a whole fsim/SU(4) layer segment in ONE global pass.
constexpr int QA_MAX_BATCH_2Q = 6;

template <typename R> struct Batch2qLdsArgs {
    cplx<R> m[16 * QA_MAX_BATCH_2Q]; // row-major 4x4 per pair, basis |q2 q1>
    bitCapInt p1[QA_MAX_BATCH_2Q];   // pow2(q1) (low bit of the pair index)
    bitCapInt p2[QA_MAX_BATCH_2Q];   // pow2(q2) (high bit)
    int k;
    bitCapInt maxQPower;
};

template <typename R>
void launchMtrx2qBatchLds(cplx<R>* sv, const Batch2qLdsArgs<R>& a, hipStream_t stream);

// general global two-qubit 4x4 apply (register orbit of 4 amplitudes; any
// qubit positions) — the reference decomposes SU(4) into gate strings, this
// build applies it in ONE pass.
template <typename R> struct Gate4x4Args {
    cplx<R> m[16]; // row-major, basis |q2 q1>
    bitCapInt p1;  // pow2(min qubit)
    bitCapInt p2;  // pow2(max qubit)
    bitCapInt maxI; // maxQPower >> 2
};

template <typename R>
void launchMtrx2q(cplx<R>* sv, const Gate4x4Args<R>& a, hipStream_t stream);

// dense k-qubit gate, 1 <= k <= QA_MTRXN_MAX, any targets, controls or
// anti-controls: ONE read-modify-write pass through an LDS tile whose address
// bits are the targets plus the lowest other bits (mtrxn_plan.hpp). The matrix
// is in the basis of the ascending targets; k <= 3 reads it from `m` in the
// kernel arguments, k >= 4 from `dm` (device memory, 4^k entries).
template <typename R> struct MtrxNArgs {
    MtrxNGeom g;
    cplx<R> m[64];
};

template <typename R>
void launchMtrxN(cplx<R>* sv, const cplx<R>* dm, const MtrxNArgs<R>& a, hipStream_t stream);

// TWO disjoint 4x4s in ONE full-state pass (16-amplitude orbits — the same
// register-orbit budget the 4-column QFT kernel proved runs at full HBM
// bandwidth). Matrices row-major in |q2 q1> basis with powers pre-sorted
// per gate (pA1<pA2, pB1<pB2); all four bit positions distinct.
template <typename R> struct Gate4x4Pair2Args {
    cplx<R> mA[16];
    cplx<R> mB[16];
    bitCapInt pA1, pA2, pB1, pB2;
    bitCapInt sorted4[4]; // the four powers ascending (orbit insertion)
    bitCapInt orbits;     // maxQPower >> 4
};

template <typename R>
void launchMtrx2qPair2(cplx<R>* sv, const Gate4x4Pair2Args<R>& a, hipStream_t stream);

// batched disjoint CNOTs: a whole layer of k control/target pairs (no qubit
// repeated) applied as ONE in-place permutation pass — amp[i] swaps with
// amp[i ^ xm(i)] where xm(i) XORs tPow[j] for every set control bit. One
// full-state RMW replaces k half-state passes.
constexpr int QA_MAX_BATCH_CNOT = 16;

struct CnotBatchArgs {
    bitCapInt cPow[QA_MAX_BATCH_CNOT];
    bitCapInt tPow[QA_MAX_BATCH_CNOT];
    int k;
    bitCapInt maxI; // full state size
};

template <typename R>
void launchCnotBatch(cplx<R>* sv, const CnotBatchArgs& a, hipStream_t stream);

// batched controlled-phase pairs: amp[i] *= exp(i * sum_j angle_j) over pairs
// with both bits set — one diagonal pass applies a whole CZ/CPhase layer
// (pairs may share qubits; diagonal ops commute).
struct CPhasePairsArgs {
    bitCapInt cPow[QA_MAX_BATCH_CNOT];
    bitCapInt tPow[QA_MAX_BATCH_CNOT];
    double angle[QA_MAX_BATCH_CNOT];
    int k;
    bitCapInt maxI;
};

template <typename R>
void launchCPhasePairs(cplx<R>* sv, const CPhasePairsArgs& a, hipStream_t stream);

// fully fused QFT column (H + the column's phase ramp in one pass);
// pre=false: QFT order (H then ramp), pre=true: IQFT order (ramp then H)
template <typename R>
void launchQftColumn(cplx<R>* sv, bitCapInt maxQPower, bitLenInt rampStart, bitLenInt col,
    bitCapInt tPow, int sign, bool pre, hipStream_t stream);

// contiguous per-chunk |amp|^2 sums (inverse-CDF sampling support):
// sums[c] = sum over [c*chunkLen, (c+1)*chunkLen)
template <typename R>
void launchChunkSums(
    const cplx<R>* sv, bitCapInt nChunks, bitCapInt chunkLen, double* sumsDev, hipStream_t stream);

// complex inner product <b|a>: per-block partial (re, im) pairs
template <typename R>
int launchInner(const cplx<R>* a, const cplx<R>* b, bitCapInt maxI, double* partialsRe,
    double* partialsIm, hipStream_t stream);

// marginal probabilities of the [start, start+length) register:
// probs[p] += |amp|^2 over all amplitudes with register == p  (probsDev zeroed
// by caller). Single pass, LDS histogram when 2^length <= 2048.
template <typename R>
void launchPartProbs(const cplx<R>* sv, bitCapInt maxQPower, bitLenInt start, bitLenInt length,
    double* probsDev, hipStream_t stream);

} // namespace qrack_amd
