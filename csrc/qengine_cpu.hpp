// qrack_amd — CPU Schrödinger state-vector engine.
//
// Capability parity target: /root/reference/include/qengine_cpu.hpp +
// /root/reference/src/qengine/{state,arithmetic,utility}.cpp. New design:
// dense 64-byte-aligned amplitude array + the shared ThreadPool ParallelFor;
// the full ALU family runs as out-of-place permutation copies.
#pragma once

#include "common/parallel_for.hpp"
#include "qengine.hpp"

namespace qrack_amd {

template <typename R> class QEngineCPU;
template <typename R> using QEngineCPUPtr = std::shared_ptr<QEngineCPU<R>>;

template <typename R> class QEngineCPU : public QEngine<R>, public ParallelFor {
protected:
    using QInterface<R>::qubitCount;
    using QInterface<R>::maxQPower;
    using QInterface<R>::doNormalize;
    using QInterface<R>::amplitudeFloor;
    using QEngine<R>::runningNorm;

    std::vector<cplx<R>> stateVec;

public:
    QEngineCPU(bitLenInt qBitCount, bitCapInt initState = 0u, RngPtr rgp = nullptr,
        bool doNorm = true, R normThresh = eps<R>::value,
        cplx<R> initPhase = cplx<R>((R)1, (R)0));

    cplx<R>* Amplitudes() { return stateVec.data(); }

    // ---- state access ----
    void SetQuantumState(const cplx<R>* inputState) override;
    void GetQuantumState(cplx<R>* outputState) override;
    void GetProbs(R* outputProbs) override;
    cplx<R> GetAmplitude(bitCapInt perm) override { return stateVec[perm]; }
    void SetAmplitude(bitCapInt perm, cplx<R> amp) override { stateVec[perm] = amp; }
    void SetPermutation(bitCapInt perm, cplx<R> phase = cplx<R>((R)1, (R)0)) override;

    // ---- engine primitives ----
    void Apply2x2(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
        const std::vector<bitCapInt>& qPowersSorted) override;
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
    void Mtrx1qBatch(const std::vector<bitLenInt>& targets, const std::vector<cplx<R>>& mtrxs) override;
    void CnotBatch(
        const std::vector<bitLenInt>& controls, const std::vector<bitLenInt>& targets) override;
    void CPhasePairs(const std::vector<bitLenInt>& controls, const std::vector<bitLenInt>& targets,
        const std::vector<double>& angles) override;
    void Mtrx2q(const cplx<R>* m16, bitLenInt q1, bitLenInt q2) override;
    // dense k-qubit gate: one sweep over the orbits of the control subspace
    void MtrxN(const std::vector<bitLenInt>& qubits, const cplx<R>* mtrx,
        const std::vector<bitLenInt>& controls = {}, bool anti = false) override;
    void QftColumnGeneral(bitLenInt target, double scale, bitLenInt rampStart,
        bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
        const std::vector<uint64_t>& sWeights, double phase0, bool pre) override;
    void QFT(bitLenInt start, bitLenInt length, bool trySeparate = false) override;
    void IQFT(bitLenInt start, bitLenInt length, bool trySeparate = false) override;
    void PhaseRamp(R scale, bitLenInt rampStart, bitLenInt rampBits, bitCapInt condPower) override;
    void PhaseRampGeneral(R scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
        const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights,
        bitCapInt condPower) override;

    // ---- probability / measurement ----
    R Prob(bitLenInt q) override;
    R ProbAll(bitCapInt perm) override { return norm(stateVec[perm]); }
    R ProbMask(bitCapInt mask, bitCapInt permutation) override;
    R ProbReg(bitLenInt start, bitLenInt length, bitCapInt permutation) override;
    R ProbParity(bitCapInt mask) override;
    bool ForceMParity(bitCapInt mask, bool result, bool doForce = true) override;
    bitCapInt MAll() override;
    std::map<bitCapInt, int> MultiShotMeasureMask(
        const std::vector<bitCapInt>& qPowers, unsigned shots) override;
    double ExpectationBitsFactorized(const std::vector<bitLenInt>& bits,
        const std::vector<bitCapInt>& perms, bitCapInt offset = 0) override;
    double VarianceBitsAll(const std::vector<bitLenInt>& bits, bitCapInt offset = 0) override;
    // Pauli strings and sums: one read-only pass per distinct X/Y mask
    double PauliExpectation(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double ExpectationPauliAll(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double VariancePauliAll(
        const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis) override;
    double ExpectationPauliSum(const std::vector<PauliTerm>& terms) override;
    // reduced density matrices: one read-only pass, no state copy; private
    // per-worker matrices folded in worker order, so a repeat is bit-identical
    void GetReducedDensityMatrix(const std::vector<bitLenInt>& qubits, cplx<double>* out) override;
    void GetReducedDensityMatrix(bitLenInt q, cplx<R>* out) override;
    // Pauli rotations and Pauli-sum evolution: one in-place sweep per planned
    // pass (pauliEvolvePlan, qengine.hpp), weights and angles in double
    void PauliRotation(const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis,
        double theta) override;
    void EvolvePauliSum(
        const std::vector<PauliTerm>& terms, double time, int steps = 1, int order = 1) override;
    // Brakets, H|psi> and the adjoint gradient: the pair walk of the Pauli
    // sums, one sweep per X/Y mask; complex sums are private per worker and
    // added in worker order. The gradient keeps one second amplitude array.
    cplx<double> PauliSumBraket(QInterfacePtr<R> bra, const std::vector<PauliTerm>& terms) override;
    void PauliSumApplyInto(const std::vector<PauliTerm>& terms, QInterfacePtr<R> dest) override;
    double AdjointGradient(const std::vector<AdjointOp<R>>& ops, const std::vector<PauliTerm>& terms,
        std::vector<double>& grad) override;
    // Krylov calls (krylov.hpp): a Lanczos step is one sweep per X/Y mask that
    // also sums alpha's share, and one finishing sweep that returns beta^2;
    // sums are private per worker and added in worker order. The two calls
    // that need the basis keep dim amplitude arrays, the tridiagonal three.
    void LanczosTridiagonal(const std::vector<PauliTerm>& terms, int dim, std::vector<double>& alpha,
        std::vector<double>& beta) override;
    double KrylovEvolvePauliSum(
        const std::vector<PauliTerm>& terms, double time, int dim = 16, int steps = 1) override;
    std::pair<double, double> LanczosGroundState(
        const std::vector<PauliTerm>& terms, int dim = 32, bool prepare = false) override;
    // krylovEigenDrive around plain sweeps: H v_j through pauliApplyRun on
    // scaled weights, then per chunk one Kahan sum per inner product and one
    // update sweep. dim amplitude arrays, dim + 1 when maxRestarts > 0.
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

    // ---- ALU (parity: qheader_alu.cl kernel family) ----
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
    // Run `perm` over all indices (optionally restricted by controlMask all-set),
    // writing nState[f(i)] = state[i]; f must be a bijection on the iterated set.
    void PermutationOp(const std::function<bitCapInt(bitCapInt)>& f);
    void ControlledPermutationOp(
        bitCapInt controlMask, const std::function<bitCapInt(bitCapInt)>& f);
    // Copy of the state with the fully-controlled subspace cleared: the start
    // vector for controlled ops that map a sub-domain (carry/out register |0>)
    // of that subspace, so no unmapped source slot keeps a stale amplitude.
    std::vector<cplx<R>> UncontrolledCopy(bitCapInt controlMask);
    bitCapInt SampleOnce();
    void QftColumn(bitLenInt start, bitLenInt col, int sign, bool pre);
    double pauliGroupSum(const PauliGroup& g);
    void pauliEvolveRun(const PauliCanonSum& c, const PauliEvolvePlan& plan);
    cplx<double> pauliBraketRun(const PauliCanonSum& c, const cplx<R>* bra, const cplx<R>* psi);
    void pauliApplyRun(const PauliCanonSum& c, const cplx<R>* psi, cplx<R>* dest);
    // <lam|P|psi> for the one string of g, then exp(-i angle P) on both arrays
    cplx<double> pauliAdjointStep(const PauliGroup& g, double angle, cplx<R>* psi, cplx<R>* lam);
    // dest <- s H u - b prev - a u with a = s^2 A, A = Re <u | s H u - b prev>
    // (prev may be null when b == 0; dest keeps s H u - b prev when !store);
    // returns (A, ||s H u - b prev - a u||^2)
    std::pair<double, double> krylovStep(const PauliCanonSum& c, double s, double b, const cplx<R>* u,
        const cplx<R>* prev, cplx<R>* dest, bool store);
    // Lanczos(dim) from the state: step j writes bufs[(j - 1) % bufs.size()]
    KrylovRun lanczosRun(const PauliCanonSum& c, int dim, std::vector<std::vector<cplx<R>>>& bufs,
        const char* what);
    // state <- coef[0] state + sum_j coef[j] bufs[j - 1]
    void krylovCombine(const std::vector<cplx<double>>& coef, const std::vector<std::vector<cplx<R>>>& bufs);
    bool pauliStringNative(const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis,
        const char* what, double& value);

};

} // namespace qrack_amd
