// qrack_amd — MI355X (gfx950) Schrödinger state-vector engine.
//
// Capability parity target: /root/reference/include/qengine_opencl.hpp +
// /root/reference/src/qengine/opencl.cpp (and its CUDA twin) — one HIP
// engine, no dual backend. New design:
//  - amplitudes live in HBM3E via hipMalloc (288 GB/GPU budget; per-device
//    allocation accounting with QRACK_MAX_ALLOC_MB cap, throwing
//    std::bad_alloc for the QUnit ACE ladder);
//  - one HIP stream per engine instance; every gate launch is asynchronous,
//    host sync happens only at probability/amplitude reads (the reference's
//    QueueItem machinery collapses into HIP stream semantics);
//  - reductions return per-block partials summed on host;
//  - ALU ops ping-pong between the state buffer and a lazily-allocated
//    scratch buffer of equal size.
#pragma once

#include "../qengine.hpp"
#include "kernels.hpp"
#include "qft_plan.hpp"

#include <hip/hip_runtime.h>

namespace qrack_amd {

#define QA_HIP_CHECK(expr)                                                                          \
    do {                                                                                            \
        hipError_t qa_err_ = (expr);                                                                \
        if (qa_err_ == hipErrorOutOfMemory) throw std::bad_alloc();                                 \
        if (qa_err_ != hipSuccess)                                                                  \
            throw QrackError(std::string("HIP error: ") + hipGetErrorString(qa_err_) + " at " +     \
                __FILE__ + ":" + std::to_string(__LINE__));                                         \
    } while (0)

// Per-device allocation bookkeeping (parity: OCLEngine activeAllocSizes,
// oclengine.hpp:322-377).
class HipDeviceTracker {
public:
    static HipDeviceTracker& instance();
    int deviceCount();
    size_t totalMem(int dev);
    size_t activeAlloc(int dev);
    void add(int dev, size_t bytes);   // throws std::bad_alloc over cap
    void sub(int dev, size_t bytes);
    int defaultDevice();

private:
    HipDeviceTracker();
    std::vector<size_t> totals_;
    std::vector<std::atomic<size_t>> active_;
    std::vector<size_t> caps_;
    int count_ = 0;
};

// opt-in per-op wall-clock profiler (QRACK_PROFILE=1): synchronous timing
// around each launch category, reported via qrack_amd.profile_report()
// (aux-subsystem parity: SURVEY.md §5 tracing — HIP-event/QueueItem timing)
struct HipProfiler {
    static bool Enabled();
    static void Add(const char* op, double ms);
    static std::map<std::string, std::pair<uint64_t, double>> Report();
    static void Reset();
};

class HipProfScope {
public:
    HipProfScope(const char* op, hipStream_t stream);
    ~HipProfScope();

private:
    const char* op_;
    hipStream_t stream_;
    double t0_ = 0;
};

template <typename R> class QEngineHIP;
template <typename R> using QEngineHIPPtr = std::shared_ptr<QEngineHIP<R>>;

template <typename R> class QEngineHIP : public QEngine<R> {
protected:
    using QInterface<R>::qubitCount;
    using QInterface<R>::maxQPower;
    using QInterface<R>::doNormalize;
    using QInterface<R>::amplitudeFloor;
    using QEngine<R>::runningNorm;

    int deviceId;
    hipStream_t stream;
    cplx<R>* dScratch = nullptr; // same size as the state buffer, lazily allocated
    double* dPartials = nullptr; // reduce partials (QA-reduce grid max + argmax idx)
    bitCapInt* dIdx = nullptr;
    std::vector<double> hPartials;
    // host tables that a kernel reads (multiplexer matrices and control powers,
    // ALU lookup tables): one engine-owned device buffer, grown on demand
    unsigned char* dAux_ = nullptr;
    size_t auxBytes_ = 0;
    std::vector<unsigned char> hAux_;
    // stage `bytes` of hAux_ into dAux_ in stream order; returns dAux_
    unsigned char* uploadAux(size_t bytes);
    unsigned char* uploadTable(const unsigned char* values, size_t bytes);
    void releaseAux();

public:
    QEngineHIP(bitLenInt qBitCount, bitCapInt initState = 0u, RngPtr rgp = nullptr,
        bool doNorm = true, R normThresh = eps<R>::value, int64_t devId = -1,
        cplx<R> initPhase = cplx<R>((R)1, (R)0));
    ~QEngineHIP() override;

    int DeviceId() const { return deviceId; }
    hipStream_t Stream() const { return stream; }
    // raw views for code the engine cannot see (dlpack, the dist pager):
    // they count as writes, and tile sums are never trusted again afterwards
    cplx<R>* DeviceBuffer() { return externState(); }
    uintptr_t DevicePtr() { return (uintptr_t)externState(); }

    void Finish() override { QA_HIP_CHECK(hipStreamSynchronize(stream)); }
    bool isFinished() override { return hipStreamQuery(stream) == hipSuccess; }
    void SetDevice(int64_t devId) override;
    int64_t GetDevice() const override { return deviceId; }

    // ---- state access ----
    void SetQuantumState(const cplx<R>* inputState) override;
    void GetQuantumState(cplx<R>* outputState) override;
    cplx<R> GetAmplitude(bitCapInt perm) override;
    void SetAmplitude(bitCapInt perm, cplx<R> amp) override;
    void SetPermutation(bitCapInt perm, cplx<R> phase = cplx<R>((R)1, (R)0)) override;

    // ---- engine primitives ----
    void Apply2x2(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
        const std::vector<bitCapInt>& qPowersSorted) override;
    void Mtrx1qBatch(const std::vector<bitLenInt>& targets, const std::vector<cplx<R>>& mtrxs) override;
    void CnotBatch(
        const std::vector<bitLenInt>& controls, const std::vector<bitLenInt>& targets) override;
    void CPhasePairs(const std::vector<bitLenInt>& controls, const std::vector<bitLenInt>& targets,
        const std::vector<double>& angles) override;
    void FSimBatch(const std::vector<R>& thetas, const std::vector<R>& phis,
        const std::vector<bitLenInt>& q1s, const std::vector<bitLenInt>& q2s) override;
    void Mtrx2q(const cplx<R>* m16, bitLenInt q1, bitLenInt q2) override;
    void Mtrx2qBatch(const std::vector<cplx<R>>& ms, const std::vector<bitLenInt>& q1s,
        const std::vector<bitLenInt>& q2s) override;
    // dense k-qubit gate: one tiled pass (k_mtrx_n) laid out by mtrxnPlan
    // (mtrxn_plan.hpp); k = 1 and the uncontrolled k = 2 go to the kernels
    // that already serve them
    void MtrxN(const std::vector<bitLenInt>& qubits, const cplx<R>* mtrx,
        const std::vector<bitLenInt>& controls = {}, bool anti = false) override;
    void ApplyM(bitCapInt regMask, bitCapInt result, cplx<R> nrm) override;
    void GetAmplitudePage(cplx<R>* pagePtr, bitCapInt offset, bitCapInt length) override;
    void SetAmplitudePage(const cplx<R>* pagePtr, bitCapInt offset, bitCapInt length) override;
    void SetAmplitudePage(
        QEnginePtr<R> pageEnginePtr, bitCapInt srcOffset, bitCapInt dstOffset, bitCapInt length) override;
    void ShuffleBuffers(QEnginePtr<R> engine) override;
    void ZeroAmplitudes() override;
    void CopyStateVec(QEnginePtr<R> src) override;
    bool IsZeroAmplitude() override;

    // ---- fast paths ----
    void XMask(bitCapInt mask) override;
    void ZMask(bitCapInt mask) override;
    void PhaseParity(R radians, bitCapInt mask) override;
    void UniformlyControlledSingleBit(
        const std::vector<bitLenInt>& controls, bitLenInt target, const cplx<R>* mtrxs) override;
    void ROL(bitLenInt shift, bitLenInt start, bitLenInt length) override;
    // fused QFT: per column, ONE phase-ramp kernel replaces the
    // controlled-phase ladder (O(n) full-state passes instead of O(n^2/2))
    void QFT(bitLenInt start, bitLenInt length, bool trySeparate = false) override;
    void IQFT(bitLenInt start, bitLenInt length, bool trySeparate = false) override;
    void PhaseRamp(R scale, bitLenInt rampStart, bitLenInt rampBits, bitCapInt condPower) override;
    void PhaseRampGeneral(R scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
        const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights,
        bitCapInt condPower) override;
    void QftColumnGeneral(bitLenInt target, double scale, bitLenInt rampStart,
        bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
        const std::vector<uint64_t>& sWeights, double phase0, bool pre) override;
    // TWO generalized columns in one pass (distributed pager local ladder):
    // targetHi's column (scale, ramp EXCLUDING targetLo's bit) then
    // targetLo's column (2*scale on the same ramp bits); per-column
    // meta-page scalars phase0Hi/phase0Lo
    void QftColumn2General(bitLenInt targetHi, bitLenInt targetLo, double scale,
        bitLenInt rampStart, bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
        const std::vector<uint64_t>& sWeights, double phase0Hi, double phase0Lo, bool pre);
    // Pipelined-exchange building block (distributed pager): fused top-target
    // column over pair rows [itLo, itHi), one pair side read straight from
    // the RCCL receive buffer `recvPtr` (device pointer, chunk-local), and the
    // launch placed on `extStream` (torch's current HIP stream) so per-chunk
    // compute interleaves with the in-flight NCCL chunks. recvIsLow: received
    // chunk is the target=0 side (true on the high page of an exchange).
    void QftColumnTopRange(double scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
        const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights, double phase0,
        bool pre, uint64_t itLo, uint64_t itHi, uintptr_t recvPtr, bool recvIsLow,
        uintptr_t extStream);

    // ---- probability / measurement ----
    R Prob(bitLenInt q) override;
    R ProbAll(bitCapInt perm) override { return norm(GetAmplitude(perm)); }
    R ProbMask(bitCapInt mask, bitCapInt permutation) override;
    R ProbReg(bitLenInt start, bitLenInt length, bitCapInt permutation) override;
    R ProbParity(bitCapInt mask) override;
    bool ForceMParity(bitCapInt mask, bool result, bool doForce = true) override;
    bitCapInt MAll() override;
    std::map<bitCapInt, int> MultiShotMeasureMask(
        const std::vector<bitCapInt>& qPowers, unsigned shots) override;
    bitCapInt HighestProbAll() override;
    double ExpectationBitsFactorized(const std::vector<bitLenInt>& bits,
        const std::vector<bitCapInt>& perms, bitCapInt offset = 0) override;
    double VarianceBitsAll(const std::vector<bitLenInt>& bits, bitCapInt offset = 0) override;
    // Pauli strings and sums: one read-only pass per distinct X/Y mask, no
    // clone, no scratch, one host sync per call
    double PauliExpectation(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double ExpectationPauliAll(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double VariancePauliAll(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double ExpectationPauliSum(const std::vector<PauliTerm>& terms) override;
    // reduced density matrices: the launches of rdmPassPlan (rdm_plan.hpp),
    // read-only, no clone, no scratch; a pending basis state is answered on
    // the host. The single-qubit form is the k = 1 case.
    void GetReducedDensityMatrix(const std::vector<bitLenInt>& qubits, cplx<double>* out) override;
    void GetReducedDensityMatrix(bitLenInt q, cplx<R>* out) override;
    // Pauli rotations and Pauli-sum evolution: one in-place read-and-write
    // pass per planned pass (pauliEvolvePlan, qengine.hpp), no host sync
    void PauliRotation(const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis,
        double theta) override;
    void EvolvePauliSum(
        const std::vector<PauliTerm>& terms, double time, int steps = 1, int order = 1) override;
    // <bra|H|this>: one read-only launch per (X/Y mask, chunk of terms) over
    // both vectors, block partials folded on the device, one copy and one
    // host sync per call. A bra that is no HIP engine on this device is staged
    // as SumSqrDiff stages its operand.
    cplx<double> PauliSumBraket(QInterfacePtr<R> bra, const std::vector<PauliTerm>& terms) override;
    // dest <- H|this>: the same launches; the first writes dest, the rest
    // accumulate into it. dest is a HIP engine on this device.
    void PauliSumApplyInto(const std::vector<PauliTerm>& terms, QInterfacePtr<R> dest) override;
    // Adjoint gradient with one extra state-sized buffer (peak: two states).
    // Forward pass, lambda = H psi, then the backward sweep on one stream with
    // no host sync: a trainable rotation is ONE fused launch over both
    // vectors, everything else is the existing launch on each. The energy and
    // every <lambda|P|psi> come back in one copy at the end. (A gate on more
    // than 3 qubits stages its matrix through the aux buffer, which waits for
    // the stream.)
    double AdjointGradient(const std::vector<AdjointOp<R>>& ops, const std::vector<PauliTerm>& terms,
        std::vector<double>& grad) override;
    // Krylov calls (krylov.hpp), all through lanczosRun. A Lanczos step is L
    // fused apply launches and one finish, (3L + 3) state sizes of traffic,
    // and one host sync that brings (alpha, beta^2) back for the next scale;
    // the basis stays unnormalised and no pass exists only to scale. The
    // tridiagonal rotates three buffers (peak: 4 states); the evolution and
    // the preparing ground state keep u_2..u_dim and a work buffer (peak:
    // dim + 1 states), taken up front so that a refusal leaves the state alone.
    void LanczosTridiagonal(const std::vector<PauliTerm>& terms, int dim, std::vector<double>& alpha,
        std::vector<double>& beta) override;
    double KrylovEvolvePauliSum(
        const std::vector<PauliTerm>& terms, double time, int dim = 16, int steps = 1) override;
    std::pair<double, double> LanczosGroundState(
        const std::vector<PauliTerm>& terms, int dim = 32, bool prepare = false) override;
    // krylovEigenDrive (krylov.hpp). A step at basis size j is L apply
    // launches (the first writes w without reading it), then the block
    // orthogonalisation: krylovOrthLaunches(j) launches of k_krylov_orth, whose
    // coefficients stay on the device, (3j + 5) state sizes for j <= 16; then
    // one copy of h and beta^2 and one host sync. A restart is one in-place
    // k_krylov_rotate, (k + kp) state sizes, and a pointer swap. Launches of a
    // call: applies * L krylov_apply, the sum of krylovOrthLaunches(j) over
    // its steps krylov_orth, restarts krylov_rotate, and krylov_combine only
    // with prepare >= 0. dim buffers besides the state, dim + 1 with
    // maxRestarts > 0 (a later cycle's dim vectors and its w are all the
    // call's own), taken up front.
    KrylovEigenResult LanczosLowestStates(const std::vector<PauliTerm>& terms, int nev = 2, int dim = 16,
        double tol = 0.0, int maxRestarts = 64, int prepare = -1) override;

    // ---- structural ----
    using QInterface<R>::Compose;
    bitLenInt Compose(QInterfacePtr<R> toCopy, bitLenInt start) override;
    void Decompose(bitLenInt start, QInterfacePtr<R> dest) override;
    void Dispose(bitLenInt start, bitLenInt length) override;
    void Dispose(bitLenInt start, bitLenInt length, bitCapInt disposedPerm) override;
    bitLenInt Allocate(bitLenInt start, bitLenInt length) override;
    QInterfacePtr<R> Clone() override;

    // ---- norm ----
    void UpdateRunningNorm(R norm_thresh = (R)-1) override;
    void NormalizeState(R nrm = (R)-1, R norm_thresh = (R)-1, R phaseArg = 0) override;
    double SumSqrDiff(QInterfacePtr<R> other) override;

    // ---- ALU ----
    void INC(bitCapInt toAdd, bitLenInt start, bitLenInt length) override;
    void CINC(bitCapInt toAdd, bitLenInt start, bitLenInt length,
        const std::vector<bitLenInt>& controls) override;
    void INCC(bitCapInt toAdd, bitLenInt start, bitLenInt length, bitLenInt carryIndex) override;
    void DECC(bitCapInt toSub, bitLenInt start, bitLenInt length, bitLenInt carryIndex) override;
    void INCS(bitCapInt toAdd, bitLenInt start, bitLenInt length, bitLenInt overflowIndex) override;
    void INCBCD(bitCapInt toAdd, bitLenInt start, bitLenInt length) override;
    void MUL(bitCapInt toMul, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length) override;
    void DIV(bitCapInt toDiv, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length) override;
    void MULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length) override;
    void IMULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length) override;
    void POWModNOut(bitCapInt base, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length) override;
    void CMUL(bitCapInt toMul, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length,
        const std::vector<bitLenInt>& controls) override;
    void CDIV(bitCapInt toDiv, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length,
        const std::vector<bitLenInt>& controls) override;
    void CMULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length, const std::vector<bitLenInt>& controls) override;
    void CIMULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length, const std::vector<bitLenInt>& controls) override;
    void CPOWModNOut(bitCapInt base, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
        bitLenInt length, const std::vector<bitLenInt>& controls) override;
    bitCapInt IndexedLDA(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
        bitLenInt valueLength, const unsigned char* values, bool resetValue = true) override;
    bitCapInt IndexedADC(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
        bitLenInt valueLength, bitLenInt carryIndex, const unsigned char* values) override;
    bitCapInt IndexedSBC(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
        bitLenInt valueLength, bitLenInt carryIndex, const unsigned char* values) override;
    void Hash(bitLenInt start, bitLenInt length, const unsigned char* values) override;
    void PhaseFlipIfLess(bitCapInt greaterPerm, bitLenInt start, bitLenInt length) override;
    void CPhaseFlipIfLess(
        bitCapInt greaterPerm, bitLenInt start, bitLenInt length, bitLenInt flagIndex) override;

protected:
    cplx<R>* allocDev(bitCapInt nAmps);
    void freeDev(cplx<R>* p, bitCapInt nAmps);
    void ensureScratch();
    void releaseScratch();
    void swapScratch(); // state <-> scratch
    void resizeState(bitCapInt nAmps, cplx<R>* newBuf); // replace buffer
    double reduceSum(int op, const ReduceArgs& a);
    double pauliGroupsSum(const std::vector<PauliGroup>& groups);
    void pauliEvolveRun(const PauliCanonSum& c, const PauliEvolvePlan& plan);
    // dst <- (identity + groups) src, one profiled launch per (group, chunk)
    void pauliApplyRun(const PauliCanonSum& c, const cplx<R>* src, cplx<R>* dst);
    // exp(-i angle P) for the one string of g on a raw buffer (a state or the
    // adjoint sweep's second vector), through the evolution launcher
    void pauliRotateBuffer(cplx<R>* buf, const PauliGroup& g, double angle);
    // raw accounted state-sized buffers of one Krylov call, freed on every way out
    struct KrylovBuffers {
        QEngineHIP<R>* self;
        std::vector<cplx<R>*> p;
        explicit KrylovBuffers(QEngineHIP<R>* s)
            : self(s)
        {
        }
        KrylovBuffers(const KrylovBuffers&) = delete;
        KrylovBuffers& operator=(const KrylovBuffers&) = delete;
        ~KrylovBuffers()
        {
            for (cplx<R>* q : p) self->freeDev(q, self->maxQPower);
        }
        void take(size_t n)
        {
            p.reserve(n);
            while (p.size() < n) p.push_back(self->allocDev(self->maxQPower));
        }
    };
    // Lanczos(dim) from the state: step j writes bufs[(j - 1) % bufs.size()]
    KrylovRun lanczosRun(const PauliCanonSum& c, int dim, const std::vector<cplx<R>*>& bufs, const char* what);
    // state <- coef[0] state + sum_j coef[j] bufs[j - 1], in as many launches
    // as KRYLOV_COMBINE_MAX_VECTORS sources each take
    void krylovCombine(const std::vector<cplx<double>>& coef, const std::vector<cplx<R>*>& bufs);
    // device slots for `n` (re, im) results of the pair-walk reductions
    double* pairResults(size_t n);
    void releasePairResults();
    // string with X/Y factors -> value; false when the generic lowering must answer
    bool pauliStringNative(const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis,
        const char* what, double& value);
    // block partials and per-launch results of the reduced-density-matrix
    // passes: accounted like the state, allocated on first use, grown on demand
    double* rdmBuffer(size_t doubles);
    void releaseRdm();
    std::pair<double, bitCapInt> argMax();
    std::vector<double> partProbs(bitLenInt start, bitLenInt length);
    bitCapInt sampleOnce(const std::vector<double>& chunkSums, bitCapInt chunkLen, double r,
        std::vector<cplx<R>>& hostChunk, bitCapInt& cachedChunk);
    std::vector<double> chunkSums(bitCapInt& chunkLenOut);
    void permuteOp(PermArgs& a, bool partialSpace, bool copyFirst);
    GateArgs<R> makeGateArgs(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
        const std::vector<bitCapInt>& qPowersSorted);

    // ---- state buffer access ----
    // The buffer is reached ONLY through these accessors, so no site can
    // see a stale buffer or leave stale tile sums behind:
    //  - rState(): read access; materialises a pending basis state and
    //    keeps the tile sums
    //  - wState(): write access; materialises and drops the tile sums
    //  - wStateAll(): the caller overwrites EVERY amplitude; drops a pending
    //    basis state without materialising it, and drops the tile sums
    const cplx<R>* rState()
    {
        materialize();
        return dState_;
    }
    cplx<R>* wState()
    {
        materialize();
        tileSumsValid_ = false;
        return dState_;
    }
    cplx<R>* wStateAll()
    {
        basisPending_ = false;
        tileSumsValid_ = false;
        return dState_;
    }
    cplx<R>* externState()
    {
        // the caller works on streams of its own: a fill queued here must
        // have landed before the pointer is handed out
        const bool wasPending = basisPending_;
        externView_ = true;
        cplx<R>* p = wState();
        if (wasPending) Finish();
        return p;
    }

private:
    void materialize(); // pending basis state -> real buffer (memset + one amplitude)
    // whole QFT/IQFT of a pending basis state as support-restricted passes
    // (qftSupportPlan); false, with nothing done, where that does not apply
    bool qftFromBasis(const std::vector<QftPass>& plan, bool inverse, int wideLowBits);
    void setStateBuffer(cplx<R>* buf); // adopt a new buffer (contents defined by the caller)
    double* tileSumsBuffer();          // lazily allocated, maxQPower >> tile bits doubles
    void releaseTileSums();
    bool tileSumsUsable() const;       // switch on, no external view taken
    // signed-zero template of the sparse last QFT pass (kernels.hpp) for an
    // nCols-column ladder, formed on first use
    const unsigned char* qftZeroTemplate(int nCols);
    void releaseQftZeroTemplate();

    cplx<R>* dState_ = nullptr;
    // lazy basis state: the state is basisPhase_·|basisPerm_> and the
    // buffer contents are undefined until materialize() or a synthesised
    // first QFT pass defines them
    bool basisPending_ = false;
    bitCapInt basisPerm_ = 0;
    cplx<R> basisPhase_ = cplx<R>((R)1, (R)0);
    // per-tile norms left by the last forward low-ladder QFT pass
    double* dTileSums_ = nullptr;
    bitCapInt tileSumsLen_ = 0;
    bool tileSumsValid_ = false;
    unsigned char* dQftZeroTpl_ = nullptr;
    int qftZeroTplCols_ = 0; // ladder length the template holds, 0: none
    bool externView_ = false; // sticky: a raw pointer escaped this engine
    double* dRdm_ = nullptr;
    size_t rdmBytes_ = 0;
    double* dPairRes_ = nullptr; // (re, im) per launch of a braket or gradient call
    size_t pairResLen_ = 0;      // in results
};

} // namespace qrack_amd
