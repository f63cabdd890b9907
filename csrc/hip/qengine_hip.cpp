// qrack_amd — HIP engine host implementation (see qengine_hip.hpp).
#include "qengine_hip.hpp"
#include "qft_plan.hpp"

#include <set>

#include "../qfactory.hpp"

#include <chrono>
#include <mutex>

#include <algorithm>
#include <cstring>

namespace qrack_amd {

template <typename R>
static void qaCheckModN(bitCapInt modN, bitLenInt length, const char* op)
{
    if (modN == 0u || modN > pow2(length)) {
        throw QrackError(std::string(op) + ": modN must be in (0, 2^length]");
    }
}


// ---- profiler ---------------------------------------------------------------

namespace {
std::mutex g_profMtx;
std::map<std::string, std::pair<uint64_t, double>> g_prof;
double nowMs()
{
    return std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now().time_since_epoch())
        .count();
}
} // namespace

bool HipProfiler::Enabled()
{
    static bool v = [] {
        const char* env = std::getenv("QRACK_PROFILE");
        return env && std::atoi(env) != 0;
    }();
    return v;
}

void HipProfiler::Add(const char* op, double ms)
{
    std::lock_guard<std::mutex> lk(g_profMtx);
    auto& e = g_prof[op];
    e.first++;
    e.second += ms;
}

std::map<std::string, std::pair<uint64_t, double>> HipProfiler::Report()
{
    std::lock_guard<std::mutex> lk(g_profMtx);
    return g_prof;
}

void HipProfiler::Reset()
{
    std::lock_guard<std::mutex> lk(g_profMtx);
    g_prof.clear();
}

HipProfScope::HipProfScope(const char* op, hipStream_t stream)
    : op_(op)
    , stream_(stream)
{
    if (!HipProfiler::Enabled()) return;
    hipStreamSynchronize(stream_);
    t0_ = nowMs();
}

HipProfScope::~HipProfScope()
{
    if (!HipProfiler::Enabled()) return;
    hipStreamSynchronize(stream_);
    HipProfiler::Add(op_, nowMs() - t0_);
}

// ---- device tracker ---------------------------------------------------------

HipDeviceTracker& HipDeviceTracker::instance()
{
    static HipDeviceTracker t;
    return t;
}

HipDeviceTracker::HipDeviceTracker()
{
    if (hipGetDeviceCount(&count_) != hipSuccess) count_ = 0;
    totals_.resize(count_);
    caps_.resize(count_);
    active_ = std::vector<std::atomic<size_t>>(count_);
    size_t capMb = 0;
    if (const char* env = std::getenv("QRACK_MAX_ALLOC_MB")) capMb = (size_t)std::atoll(env);
    for (int d = 0; d < count_; ++d) {
        hipDeviceProp_t props;
        if (hipGetDeviceProperties(&props, d) == hipSuccess) {
            totals_[d] = props.totalGlobalMem;
        }
        active_[d] = 0;
        // default cap: 15/16 of VRAM (state + equal-size scratch both fit at
        // the max paged state of 2^33 fp32 amps; reference used OclMemDenom=3)
        caps_[d] = capMb ? capMb * (1ull << 20) : (totals_[d] / 16) * 15;
    }
}

int HipDeviceTracker::deviceCount() { return count_; }
size_t HipDeviceTracker::totalMem(int dev) { return totals_.at(dev); }
size_t HipDeviceTracker::activeAlloc(int dev) { return active_.at(dev).load(); }
int HipDeviceTracker::defaultDevice()
{
    if (const char* env = std::getenv("QRACK_HIP_DEFAULT_DEVICE")) return std::atoi(env);
    return 0;
}

void HipDeviceTracker::add(int dev, size_t bytes)
{
    const size_t now = active_.at(dev).fetch_add(bytes) + bytes;
    if (now > caps_.at(dev)) {
        active_.at(dev).fetch_sub(bytes);
        throw std::bad_alloc();
    }
}

void HipDeviceTracker::sub(int dev, size_t bytes) { active_.at(dev).fetch_sub(bytes); }

// ---- ctor / alloc -----------------------------------------------------------

template <typename R>
QEngineHIP<R>::QEngineHIP(bitLenInt qBitCount, bitCapInt initState, RngPtr rgp, bool doNorm,
    R normThresh, int64_t devId, cplx<R> initPhase)
    : QEngine<R>(qBitCount, rgp, doNorm, normThresh)
{
    auto& tracker = HipDeviceTracker::instance();
    if (tracker.deviceCount() < 1) throw QrackError("no HIP device visible");
    deviceId = (devId < 0) ? tracker.defaultDevice() : (int)devId;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    dState_ = allocDev(maxQPower);
    const int maxGrid = QA_REDUCE_MAX_BLOCKS;
    QA_HIP_CHECK(hipMalloc(&dPartials, maxGrid * 2 * sizeof(double)));
    QA_HIP_CHECK(hipMalloc(&dIdx, maxGrid * sizeof(bitCapInt)));
    hPartials.resize(maxGrid * 2);
    SetPermutation(initState, initPhase);
}

template <typename R> QEngineHIP<R>::~QEngineHIP()
{
    hipStreamSynchronize(stream);
    if (dState_) freeDev(dState_, maxQPower);
    releaseScratch();
    releaseTileSums();
    releaseQftZeroTemplate();
    releaseAux();
    releaseRdm();
    releasePairResults();
    if (dPartials) hipFree(dPartials);
    if (dIdx) hipFree(dIdx);
    hipStreamDestroy(stream);
}

template <typename R> cplx<R>* QEngineHIP<R>::allocDev(bitCapInt nAmps)
{
    auto& tracker = HipDeviceTracker::instance();
    const size_t bytes = sizeof(cplx<R>) * nAmps;
    tracker.add(deviceId, bytes);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* p = nullptr;
    const hipError_t err = hipMalloc(&p, bytes);
    if (err != hipSuccess) {
        tracker.sub(deviceId, bytes);
        if (err == hipErrorOutOfMemory) throw std::bad_alloc();
        QA_HIP_CHECK(err);
    }
    return p;
}

template <typename R> void QEngineHIP<R>::freeDev(cplx<R>* p, bitCapInt nAmps)
{
    if (!p) return;
    hipFree(p);
    HipDeviceTracker::instance().sub(deviceId, sizeof(cplx<R>) * nAmps);
}

template <typename R> void QEngineHIP<R>::ensureScratch()
{
    if (!dScratch) dScratch = allocDev(maxQPower);
}

template <typename R> void QEngineHIP<R>::releaseScratch()
{
    if (dScratch) {
        freeDev(dScratch, maxQPower);
        dScratch = nullptr;
    }
}

template <typename R> void QEngineHIP<R>::swapScratch()
{
    // the scratch buffer holds the new state: whatever described the old
    // buffer no longer applies
    basisPending_ = false;
    tileSumsValid_ = false;
    std::swap(dState_, dScratch);
}

template <typename R> void QEngineHIP<R>::resizeState(bitCapInt nAmps, cplx<R>* newBuf)
{
    Finish();
    releaseScratch();
    freeDev(dState_, maxQPower);
    setStateBuffer(newBuf);
}

template <typename R> void QEngineHIP<R>::setStateBuffer(cplx<R>* buf)
{
    dState_ = buf;
    basisPending_ = false;
    // the tile-sum buffer is sized by the state: drop it with the old one
    releaseTileSums();
}

template <typename R> void QEngineHIP<R>::releaseAux()
{
    if (dAux_) hipFree(dAux_);
    dAux_ = nullptr;
    auxBytes_ = 0;
}

// The tables used to go into a fresh hipMallocAsync block per call, freed with
// hipFreeAsync after the kernel. From the second call on one engine the kernel
// could then read something other than the table just copied there: the
// multiplexer returned an all-zero state or applied matrix 0 everywhere, and
// the indexed ALU ops lost norm. A buffer the engine keeps has no such window.
// Callers wait for the stream before they refill hAux_, so that neither the
// last kernel still reads dAux_ nor the last copy still reads hAux_.
template <typename R> unsigned char* QEngineHIP<R>::uploadAux(size_t bytes)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    if (bytes > auxBytes_) {
        QA_HIP_CHECK(hipStreamSynchronize(stream));
        releaseAux();
        QA_HIP_CHECK(hipMalloc(&dAux_, bytes));
        auxBytes_ = bytes;
    }
    QA_HIP_CHECK(hipMemcpyAsync(dAux_, hAux_.data(), bytes, hipMemcpyHostToDevice, stream));
    return dAux_;
}

template <typename R> void QEngineHIP<R>::releaseRdm()
{
    if (!dRdm_) return;
    hipFree(dRdm_);
    HipDeviceTracker::instance().sub(deviceId, rdmBytes_);
    dRdm_ = nullptr;
    rdmBytes_ = 0;
}

template <typename R> double* QEngineHIP<R>::rdmBuffer(size_t doubles)
{
    const size_t bytes = doubles * sizeof(double);
    if (bytes <= rdmBytes_) return dRdm_;
    QA_HIP_CHECK(hipStreamSynchronize(stream));
    releaseRdm();
    auto& tracker = HipDeviceTracker::instance();
    tracker.add(deviceId, bytes);
    const hipError_t err = hipMalloc(&dRdm_, bytes);
    if (err != hipSuccess) {
        dRdm_ = nullptr;
        tracker.sub(deviceId, bytes);
        QA_HIP_CHECK(err);
    }
    rdmBytes_ = bytes;
    return dRdm_;
}

template <typename R> void QEngineHIP<R>::releaseTileSums()
{
    if (dTileSums_) hipFree(dTileSums_);
    dTileSums_ = nullptr;
    tileSumsLen_ = 0;
    tileSumsValid_ = false;
}

template <typename R> double* QEngineHIP<R>::tileSumsBuffer()
{
    const bitCapInt len = maxQPower >> qaLdsTileBits<R>();
    if (dTileSums_ && tileSumsLen_ != len) releaseTileSums();
    if (!dTileSums_) {
        QA_HIP_CHECK(hipMalloc(&dTileSums_, len * sizeof(double)));
        tileSumsLen_ = len;
    }
    return dTileSums_;
}

template <typename R> void QEngineHIP<R>::releaseQftZeroTemplate()
{
    if (dQftZeroTpl_) hipFree(dQftZeroTpl_);
    dQftZeroTpl_ = nullptr;
    qftZeroTplCols_ = 0;
}

template <typename R> const unsigned char* QEngineHIP<R>::qftZeroTemplate(int nCols)
{
    // the template depends on the ladder length alone, and an engine's plan
    // ends in one ladder length: formed on first use, on the engine's stream
    if (!dQftZeroTpl_) QA_HIP_CHECK(hipMalloc(&dQftZeroTpl_, QA_QFT_ZERO_TPL_BYTES));
    if (qftZeroTplCols_ != nCols) {
        qftZeroTplCols_ = 0;
        launchQftSparseZeroTemplate(dQftZeroTpl_, nCols, stream);
        qftZeroTplCols_ = nCols;
    }
    return dQftZeroTpl_;
}

namespace {
bool qaEnvSwitch(const char* name)
{
    const char* env = std::getenv(name);
    return env ? std::atoi(env) != 0 : true;
}
// QRACK_GPU_QFT_LAZYPERM=0: SetPermutation fills the buffer eagerly
bool qaLazyPerm()
{
    static const bool v = qaEnvSwitch("QRACK_GPU_QFT_LAZYPERM");
    return v;
}
// QRACK_GPU_QFT_SUMS=0: sampling always re-reads the state for its chunk sums
bool qaQftSums()
{
    static const bool v = qaEnvSwitch("QRACK_GPU_QFT_SUMS");
    return v;
}
} // namespace

template <typename R> bool QEngineHIP<R>::tileSumsUsable() const
{
    return qaQftSums() && !externView_;
}

template <typename R> void QEngineHIP<R>::materialize()
{
    if (!basisPending_) return;
    basisPending_ = false;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemsetAsync(dState_, 0, sizeof(cplx<R>) * maxQPower, stream));
    launchSetAmp<R>(dState_, basisPerm_, basisPhase_, stream);
}

template <typename R> void QEngineHIP<R>::SetDevice(int64_t devId)
{
    if (devId == deviceId || devId < 0) return;
    // migrate the state buffer to another GPU
    Finish();
    std::vector<cplx<R>> host(maxQPower);
    GetQuantumState(host.data());
    releaseScratch();
    releaseTileSums();
    releaseQftZeroTemplate();
    releaseAux();
    releaseRdm();
    releasePairResults();
    freeDev(dState_, maxQPower);
    hipStreamDestroy(stream);
    hipFree(dPartials);
    hipFree(dIdx);
    deviceId = (int)devId;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    dState_ = allocDev(maxQPower);
    QA_HIP_CHECK(hipMalloc(&dPartials, QA_REDUCE_MAX_BLOCKS * 2 * sizeof(double)));
    QA_HIP_CHECK(hipMalloc(&dIdx, QA_REDUCE_MAX_BLOCKS * sizeof(bitCapInt)));
    SetQuantumState(host.data());
}

// ---- state access -----------------------------------------------------------

template <typename R> void QEngineHIP<R>::SetQuantumState(const cplx<R>* inputState)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemcpyAsync(
        wStateAll(), inputState, sizeof(cplx<R>) * maxQPower, hipMemcpyHostToDevice, stream));
    Finish();
    runningNorm = (R)-1;
}

template <typename R> void QEngineHIP<R>::GetQuantumState(cplx<R>* outputState)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemcpyAsync(
        outputState, rState(), sizeof(cplx<R>) * maxQPower, hipMemcpyDeviceToHost, stream));
    Finish();
}

template <typename R> cplx<R> QEngineHIP<R>::GetAmplitude(bitCapInt perm)
{
    cplx<R> amp;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(
        hipMemcpyAsync(&amp, rState() + perm, sizeof(cplx<R>), hipMemcpyDeviceToHost, stream));
    Finish();
    return amp;
}

template <typename R> void QEngineHIP<R>::SetAmplitude(bitCapInt perm, cplx<R> amp)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(
        hipMemcpyAsync(wState() + perm, &amp, sizeof(cplx<R>), hipMemcpyHostToDevice, stream));
    Finish();
    runningNorm = (R)-1;
}

template <typename R> void QEngineHIP<R>::SetPermutation(bitCapInt perm, cplx<R> phase)
{
    if (norm(phase) <= 0) phase = cplx<R>(1, 0);
    if (qaLazyPerm()) {
        // lazy: record "the state is phase·|perm>" and touch nothing; the
        // first reader/writer materialises it, a QFT whose first pass is an
        // LDS kernel synthesises it instead
        basisPending_ = true;
        basisPerm_ = perm;
        basisPhase_ = phase;
        tileSumsValid_ = false;
    } else {
        QA_HIP_CHECK(hipSetDevice(deviceId));
        QA_HIP_CHECK(hipMemsetAsync(wStateAll(), 0, sizeof(cplx<R>) * maxQPower, stream));
        SetAmplitude(perm, phase);
    }
    runningNorm = (R)1;
}

template <typename R> void QEngineHIP<R>::ZeroAmplitudes()
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemsetAsync(wStateAll(), 0, sizeof(cplx<R>) * maxQPower, stream));
    runningNorm = 0;
}

template <typename R> void QEngineHIP<R>::CopyStateVec(QEnginePtr<R> src)
{
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(src.get());
    QA_HIP_CHECK(hipSetDevice(deviceId));
    if (o && o->deviceId == deviceId) {
        const cplx<R>* srcBuf = o->rState();
        o->Finish();
        QA_HIP_CHECK(hipMemcpyAsync(
            wStateAll(), srcBuf, sizeof(cplx<R>) * maxQPower, hipMemcpyDeviceToDevice, stream));
        Finish();
    } else {
        std::vector<cplx<R>> host(maxQPower);
        src->GetQuantumState(host.data());
        SetQuantumState(host.data());
    }
    runningNorm = (R)-1;
}

template <typename R> bool QEngineHIP<R>::IsZeroAmplitude()
{
    ReduceArgs a{};
    a.maxI = maxQPower;
    return reduceSum((int)ReduceOp::NORM_ALL, a) <= 0.0;
}

template <typename R>
void QEngineHIP<R>::GetAmplitudePage(cplx<R>* pagePtr, bitCapInt offset, bitCapInt length)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemcpyAsync(
        pagePtr, rState() + offset, sizeof(cplx<R>) * length, hipMemcpyDeviceToHost, stream));
    Finish();
}

template <typename R>
void QEngineHIP<R>::SetAmplitudePage(const cplx<R>* pagePtr, bitCapInt offset, bitCapInt length)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemcpyAsync(
        wState() + offset, pagePtr, sizeof(cplx<R>) * length, hipMemcpyHostToDevice, stream));
    Finish();
    runningNorm = (R)-1;
}

template <typename R>
void QEngineHIP<R>::SetAmplitudePage(
    QEnginePtr<R> pageEnginePtr, bitCapInt srcOffset, bitCapInt dstOffset, bitCapInt length)
{
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(pageEnginePtr.get());
    QA_HIP_CHECK(hipSetDevice(deviceId));
    if (o) {
        const cplx<R>* srcBuf = o->rState();
        o->Finish();
        if (o->deviceId == deviceId) {
            QA_HIP_CHECK(hipMemcpyAsync(wState() + dstOffset, srcBuf + srcOffset,
                sizeof(cplx<R>) * length, hipMemcpyDeviceToDevice, stream));
        } else {
            QA_HIP_CHECK(hipMemcpyPeerAsync(wState() + dstOffset, deviceId, srcBuf + srcOffset,
                o->deviceId, sizeof(cplx<R>) * length, stream));
        }
        Finish();
    } else {
        std::vector<cplx<R>> host(length);
        pageEnginePtr->GetAmplitudePage(host.data(), srcOffset, length);
        SetAmplitudePage(host.data(), dstOffset, length);
    }
    runningNorm = (R)-1;
}

template <typename R> void QEngineHIP<R>::ShuffleBuffers(QEnginePtr<R> engine)
{
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(engine.get());
    const bitCapInt half = maxQPower >> 1u;
    if (o && o->deviceId == deviceId) {
        cplx<R>* oBuf = o->wState();
        o->Finish();
        QA_HIP_CHECK(hipSetDevice(deviceId));
        launchShuffleSwap<R>(wState() + half, oBuf, half, stream);
        Finish();
    } else if (o) {
        // cross-device in-process: stage through a temp on this device
        cplx<R>* oBuf = o->wState();
        o->Finish();
        QA_HIP_CHECK(hipSetDevice(deviceId));
        cplx<R>* tmp = allocDev(half);
        QA_HIP_CHECK(hipMemcpyAsync(
            tmp, wState() + half, sizeof(cplx<R>) * half, hipMemcpyDeviceToDevice, stream));
        QA_HIP_CHECK(hipMemcpyPeerAsync(
            wState() + half, deviceId, oBuf, o->deviceId, sizeof(cplx<R>) * half, stream));
        QA_HIP_CHECK(hipMemcpyPeerAsync(
            oBuf, o->deviceId, tmp, deviceId, sizeof(cplx<R>) * half, stream));
        Finish();
        freeDev(tmp, half);
    } else {
        // CPU peer: stage through host
        std::vector<cplx<R>> mine(half), theirs(half);
        GetAmplitudePage(mine.data(), half, half);
        engine->GetAmplitudePage(theirs.data(), 0, half);
        SetAmplitudePage(theirs.data(), half, half);
        engine->SetAmplitudePage(mine.data(), 0, half);
    }
    runningNorm = (R)-1;
    if (o) o->runningNorm = (R)-1;
}

// ---- gates ------------------------------------------------------------------

template <typename R>
GateArgs<R> QEngineHIP<R>::makeGateArgs(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
    const std::vector<bitCapInt>& qPowersSorted)
{
    if ((int)qPowersSorted.size() > QA_MAX_SKIP_POWERS) {
        throw QrackError("too many control qubits for one gate (max 15 controls)");
    }
    GateArgs<R> a{};
    for (int i = 0; i < 4; ++i) a.m[i] = mtrx[i];
    a.offset1 = offset1;
    a.offset2 = offset2;
    a.nPowers = (int)qPowersSorted.size();
    for (int i = 0; i < a.nPowers; ++i) a.qPowers[i] = qPowersSorted[i];
    a.maxI = maxQPower >> (bitLenInt)qPowersSorted.size();
    return a;
}

template <typename R>
void QEngineHIP<R>::Apply2x2(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
    const std::vector<bitCapInt>& qPowersSorted)
{
    GateArgs<R> a = makeGateArgs(offset1, offset2, mtrx, qPowersSorted);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("apply2x2", stream);
    launchApply2x2<R>(wState(), a, stream);
}

// general two-qubit 4x4 apply: one pass (k_mtrx_2q).
template <typename R>
void QEngineHIP<R>::Mtrx2q(const cplx<R>* m, bitLenInt q1, bitLenInt q2)
{
    if (q1 == q2 || q1 >= qubitCount || q2 >= qubitCount)
        throw QrackError("Mtrx2q: bad qubit indices");
    Gate4x4Args<R> a{};
    a.p1 = pow2(std::min(q1, q2));
    a.p2 = pow2(std::max(q1, q2));
    if (q1 < q2) {
        std::copy(m, m + 16, a.m);
    } else {
        static const int permIdx[4] = { 0, 2, 1, 3 };
        for (int r = 0; r < 4; ++r) {
            for (int cc = 0; cc < 4; ++cc) a.m[4 * r + cc] = m[4 * permIdx[r] + permIdx[cc]];
        }
    }
    a.maxI = maxQPower >> 2u;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("mtrx_2q", stream);
    launchMtrx2q<R>(wState(), a, stream);
}

// dense k-qubit gate. The kernel works on the targets in ascending order, so
// the matrix's rows and columns are permuted to match on the host (no
// arithmetic). Up to 8 x 8 it travels in the kernel arguments, above that
// through the engine's aux buffer.
template <typename R>
void QEngineHIP<R>::MtrxN(const std::vector<bitLenInt>& qubits, const cplx<R>* mtrx,
    const std::vector<bitLenInt>& controls, bool anti)
{
    validateMtrxN(qubits, controls, qubitCount);
    const MtrxNPlan plan = mtrxnPlan((int)qubitCount, std::vector<int>(qubits.begin(), qubits.end()),
        std::vector<int>(controls.begin(), controls.end()), anti, (int)sizeof(R));
    if (plan.route == MtrxNRoute::Apply2x2) {
        if (controls.empty()) {
            this->Mtrx(mtrx, qubits[0]);
        } else if (anti) {
            this->MACMtrx(controls, mtrx, qubits[0]);
        } else {
            this->MCMtrx(controls, mtrx, qubits[0]);
        }
        return;
    }
    if (plan.route == MtrxNRoute::Mtrx2q) {
        this->Mtrx2q(mtrx, qubits[0], qubits[1]);
        return;
    }
    const size_t D = (size_t)1 << qubits.size();
    MtrxNArgs<R> a{};
    a.g = plan.geom;
    const cplx<R>* dm = nullptr;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    if (plan.matrixInKernarg) {
        mtrxnPermuteMatrix(plan, mtrx, a.m);
    } else {
        QA_HIP_CHECK(hipStreamSynchronize(stream)); // hAux_ and dAux_ are free again
        hAux_.resize(sizeof(cplx<R>) * D * D);
        mtrxnPermuteMatrix(plan, mtrx, reinterpret_cast<cplx<R>*>(hAux_.data()));
        dm = reinterpret_cast<const cplx<R>*>(uploadAux(sizeof(cplx<R>) * D * D));
    }
    HipProfScope prof("mtrx_n", stream);
    launchMtrxN<R>(wState(), dm, a, stream);
    runningNorm = (R)-1;
}

// batched disjoint two-qubit 4x4 layer: in-tile pairs fuse through the LDS
// kernel; the rest apply as single-pass 4x4s.
template <typename R>
void QEngineHIP<R>::Mtrx2qBatch(const std::vector<cplx<R>>& ms,
    const std::vector<bitLenInt>& q1s, const std::vector<bitLenInt>& q2s)
{
    if (q1s.size() != q2s.size() || ms.size() != 16u * q1s.size())
        throw QrackError("Mtrx2qBatch: need a 4x4 per pair");
    const bitLenInt ldsBits = (bitLenInt)qaLdsTileBits<R>();
    std::set<bitLenInt> uniq;
    bool disjoint = true;
    for (size_t i = 0; i < q1s.size(); ++i) {
        if (!uniq.insert(q1s[i]).second) disjoint = false;
        if (!uniq.insert(q2s[i]).second) disjoint = false;
    }
    std::vector<size_t> low, rest;
    for (size_t i = 0; i < q1s.size(); ++i) {
        if (disjoint && qubitCount > ldsBits && q1s[i] < ldsBits && q2s[i] < ldsBits &&
            q1s[i] != q2s[i]) {
            low.push_back(i);
        } else {
            rest.push_back(i);
        }
    }
    QA_HIP_CHECK(hipSetDevice(deviceId));
    auto permuted = [&](const cplx<R>* m, bool swapped, cplx<R>* out) {
        if (!swapped) {
            std::copy(m, m + 16, out);
            return;
        }
        static const int permIdx[4] = { 0, 2, 1, 3 };
        for (int r = 0; r < 4; ++r) {
            for (int cc = 0; cc < 4; ++cc) out[4 * r + cc] = m[4 * permIdx[r] + permIdx[cc]];
        }
    };
    for (size_t i = 0; i < low.size();) {
        const size_t k = std::min((size_t)QA_MAX_BATCH_2Q, low.size() - i);
        Batch2qLdsArgs<R> a{};
        for (size_t g = 0; g < k; ++g) {
            const size_t ix = low[i + g];
            const bool swapped = q1s[ix] > q2s[ix];
            a.p1[g] = pow2(std::min(q1s[ix], q2s[ix]));
            a.p2[g] = pow2(std::max(q1s[ix], q2s[ix]));
            permuted(&ms[16u * ix], swapped, &a.m[16 * g]);
        }
        a.k = (int)k;
        a.maxQPower = maxQPower;
        HipProfScope prof("mtrx_2q_batch_lds", stream);
        launchMtrx2qBatchLds<R>(wState(), a, stream);
        i += k;
    }
    // the rest: TWO disjoint 4x4s per pass (16-amplitude orbits)
    size_t j = 0;
    for (; disjoint && j + 1 < rest.size(); j += 2) {
        const size_t ixA = rest[j], ixB = rest[j + 1];
        Gate4x4Pair2Args<R> a{};
        permuted(&ms[16u * ixA], q1s[ixA] > q2s[ixA], a.mA);
        permuted(&ms[16u * ixB], q1s[ixB] > q2s[ixB], a.mB);
        a.pA1 = pow2(std::min(q1s[ixA], q2s[ixA]));
        a.pA2 = pow2(std::max(q1s[ixA], q2s[ixA]));
        a.pB1 = pow2(std::min(q1s[ixB], q2s[ixB]));
        a.pB2 = pow2(std::max(q1s[ixB], q2s[ixB]));
        bitCapInt s4[4] = { a.pA1, a.pA2, a.pB1, a.pB2 };
        std::sort(s4, s4 + 4);
        for (int b = 0; b < 4; ++b) a.sorted4[b] = s4[b];
        a.orbits = maxQPower >> 4u;
        HipProfScope prof("mtrx_2q_pair2", stream);
        launchMtrx2qPair2<R>(wState(), a, stream);
    }
    for (; j < rest.size(); ++j) {
        const size_t ix = rest[j];
        this->Mtrx2q(&ms[16u * ix], q1s[ix], q2s[ix]);
    }
}

// batched disjoint fsim layer: pairs whose bits BOTH sit inside the LDS
// tile fuse as 4x4s (up to 6 per single global pass); the rest apply via
// the normal swap-block + one-sided-phase path.
template <typename R>
void QEngineHIP<R>::FSimBatch(const std::vector<R>& thetas, const std::vector<R>& phis,
    const std::vector<bitLenInt>& q1s, const std::vector<bitLenInt>& q2s)
{
    if (thetas.size() != phis.size() || q1s.size() != q2s.size() || thetas.size() != q1s.size())
        throw QrackError("FSimBatch: need (theta, phi, q1, q2) per gate");
    const bitLenInt ldsBits = (bitLenInt)qaLdsTileBits<R>();
    std::set<bitLenInt> uniq;
    bool disjoint = true;
    for (size_t i = 0; i < q1s.size(); ++i) {
        if (!uniq.insert(q1s[i]).second) disjoint = false;
        if (!uniq.insert(q2s[i]).second) disjoint = false;
    }
    std::vector<size_t> low, rest;
    for (size_t i = 0; i < q1s.size(); ++i) {
        if (disjoint && qubitCount > ldsBits && q1s[i] < ldsBits && q2s[i] < ldsBits) {
            low.push_back(i);
        } else {
            rest.push_back(i);
        }
    }
    QA_HIP_CHECK(hipSetDevice(deviceId));
    for (size_t i = 0; i < low.size();) {
        const size_t k = std::min((size_t)QA_MAX_BATCH_2Q, low.size() - i);
        Batch2qLdsArgs<R> a{};
        for (size_t g = 0; g < k; ++g) {
            const size_t ix = low[i + g];
            bitLenInt qa_ = q1s[ix], qb_ = q2s[ix];
            if (qa_ > qb_) std::swap(qa_, qb_);
            a.p1[g] = pow2(qa_);
            a.p2[g] = pow2(qb_);
            // fsim(theta, phi): |01>,|10> mix by [[c,-is],[-is,c]];
            // |11> phase e^{-i phi} (basis |q2 q1| = i2 i1)
            const R ct = std::cos(thetas[ix]), st = std::sin(thetas[ix]);
            cplx<R>* m = &a.m[16 * g];
            for (int e = 0; e < 16; ++e) m[e] = cplx<R>(0, 0);
            m[0] = cplx<R>(1, 0);
            m[5] = cplx<R>(ct, 0);
            m[6] = cplx<R>(0, -st);
            m[9] = cplx<R>(0, -st);
            m[10] = cplx<R>(ct, 0);
            m[15] = polar<R>(1, -phis[ix]);
        }
        a.k = (int)k;
        a.maxQPower = maxQPower;
        HipProfScope prof("fsim_batch_lds", stream);
        launchMtrx2qBatchLds<R>(wState(), a, stream);
        i += k;
    }
    if (!rest.empty()) {
        // route high-bit fsims through Mtrx2qBatch as 4x4s: the pair-of-4x4
        // orbit kernel applies TWO per full-state pass
        std::vector<cplx<R>> ms(16u * rest.size(), cplx<R>(0, 0));
        std::vector<bitLenInt> ra, rb;
        for (size_t g = 0; g < rest.size(); ++g) {
            const size_t ix = rest[g];
            const R ct = std::cos(thetas[ix]), st = std::sin(thetas[ix]);
            cplx<R>* m = &ms[16u * g];
            m[0] = cplx<R>(1, 0);
            m[5] = cplx<R>(ct, 0);
            m[6] = cplx<R>(0, -st);
            m[9] = cplx<R>(0, -st);
            m[10] = cplx<R>(ct, 0);
            m[15] = polar<R>(1, -phis[ix]);
            ra.push_back(q1s[ix]);
            rb.push_back(q2s[ix]);
        }
        Mtrx2qBatch(ms, ra, rb);
    }
}

// batched controlled-phase pairs: one diagonal pass per layer.
template <typename R>
void QEngineHIP<R>::CPhasePairs(const std::vector<bitLenInt>& controls,
    const std::vector<bitLenInt>& targets, const std::vector<double>& angles)
{
    if (controls.size() != targets.size() || angles.size() != controls.size())
        throw QrackError("CPhasePairs: need (control, target, angle) triples");
    const size_t k = controls.size();
    if (k == 0u || k > (size_t)QA_MAX_BATCH_CNOT) {
        QInterface<R>::CPhasePairs(controls, targets, angles);
        return;
    }
    CPhasePairsArgs a{};
    for (size_t i = 0; i < k; ++i) {
        if (controls[i] >= qubitCount || targets[i] >= qubitCount)
            throw QrackError("CPhasePairs: qubit out of range");
        a.cPow[i] = pow2(controls[i]);
        a.tPow[i] = pow2(targets[i]);
        a.angle[i] = angles[i];
    }
    a.k = (int)k;
    a.maxI = maxQPower;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("cphase_pairs", stream);
    launchCPhasePairs<R>(wState(), a, stream);
}

// batched disjoint CNOTs: one permutation pass per layer (k_cnot_batch).
template <typename R>
void QEngineHIP<R>::CnotBatch(
    const std::vector<bitLenInt>& controls, const std::vector<bitLenInt>& targets)
{
    if (controls.size() != targets.size())
        throw QrackError("CnotBatch: need one target per control");
    const size_t k = controls.size();
    std::set<bitLenInt> uniq;
    for (size_t i = 0; i < k; ++i) {
        uniq.insert(controls[i]);
        uniq.insert(targets[i]);
        if (controls[i] >= qubitCount || targets[i] >= qubitCount)
            throw QrackError("CnotBatch: qubit out of range");
    }
    if (uniq.size() != 2u * k || k == 0u || k > (size_t)QA_MAX_BATCH_CNOT) {
        QInterface<R>::CnotBatch(controls, targets);
        return;
    }
    CnotBatchArgs a{};
    for (size_t i = 0; i < k; ++i) {
        a.cPow[i] = pow2(controls[i]);
        a.tPow[i] = pow2(targets[i]);
    }
    a.k = (int)k;
    a.maxI = maxQPower;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("cnot_batch", stream);
    launchCnotBatch<R>(wState(), a, stream);
}

// batched independent 1q gates: k gates in one full-state pass (k_mtrx_batch).
// fp32 fuses up to 5 gates per pass, fp64 up to 4 (register budget).
template <typename R>
void QEngineHIP<R>::Mtrx1qBatch(
    const std::vector<bitLenInt>& targets, const std::vector<cplx<R>>& mtrxs)
{
    if (mtrxs.size() != 4u * targets.size())
        throw QrackError("Mtrx1qBatch: need 4 entries per target");
    std::set<bitLenInt> uniq(targets.begin(), targets.end());
    if (uniq.size() != targets.size() || targets.size() < 2u) {
        QInterface<R>::Mtrx1qBatch(targets, mtrxs);
        return;
    }
    for (bitLenInt t : targets) {
        if (t >= qubitCount) throw QrackError("Mtrx1qBatch: target out of range");
    }
    // chunk at 4 for BOTH precisions: fp32 k=5 would leave the float4
    // vector path (k_mtrx_batch_v caps at k=4 for register budget) and the
    // scalar kernel's 8 B accesses cost more than the extra pass saves
    const size_t maxK = 4u;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    // partition: targets below the LDS tile go through the shared-memory
    // kernel (up to 12 per ONE pass, bit 0 included); the rest chunk into
    // float4 register batches of 4
    std::vector<size_t> low, high;
    const bitLenInt ldsBits = (bitLenInt)qaLdsTileBits<R>();
    if (qubitCount > ldsBits) {
        for (size_t j = 0; j < targets.size(); ++j) {
            (targets[j] < ldsBits ? low : high).push_back(j);
        }
    } else {
        for (size_t j = 0; j < targets.size(); ++j) high.push_back(j);
    }
    std::sort(low.begin(), low.end(),
        [&](size_t a, size_t b) { return targets[a] < targets[b]; });
    for (size_t i = 0; i < low.size();) {
        const size_t k = std::min((size_t)QA_MAX_BATCH_LDS, low.size() - i);
        if (k == 1u) {
            // a lone gate is cheaper on the plain pair kernel than an LDS pass
            this->Mtrx(&mtrxs[4u * low[i]], targets[low[i]]);
            ++i;
            continue;
        }
        BatchLdsArgs<R> a{};
        for (size_t g = 0; g < k; ++g) {
            a.tPow[g] = pow2(targets[low[i + g]]);
            for (int e = 0; e < 4; ++e) a.m[4u * g + e] = mtrxs[4u * low[i + g] + e];
        }
        // pad to a multiple of the kernel's register-orbit group width with
        // identity gates on spare tile bits (distinct within the last group)
        const size_t KG = (size_t)qaLdsBatchK<R>();
        size_t kp = k;
        while (kp % KG) {
            const size_t groupStart = (kp / KG) * KG;
            bitCapInt used = 0;
            for (size_t g = groupStart; g < kp; ++g) used |= a.tPow[g];
            bitCapInt pad = 1u;
            while (used & pad) pad <<= 1u;
            a.tPow[kp] = pad;
            a.m[4u * kp] = cplx<R>{ (R)1, (R)0 };
            a.m[4u * kp + 1u] = cplx<R>{ (R)0, (R)0 };
            a.m[4u * kp + 2u] = cplx<R>{ (R)0, (R)0 };
            a.m[4u * kp + 3u] = cplx<R>{ (R)1, (R)0 };
            ++kp;
        }
        // each group's targets sorted ascending (required by the kernel's
        // zero-bit insertion; 1q gates on distinct targets commute)
        for (size_t g0 = 0; g0 < kp; g0 += KG) {
            for (size_t x = g0; x < g0 + KG; ++x) {
                for (size_t y = x + 1u; y < g0 + KG; ++y) {
                    if (a.tPow[y] < a.tPow[x]) {
                        std::swap(a.tPow[x], a.tPow[y]);
                        for (int e = 0; e < 4; ++e) std::swap(a.m[4u * x + e], a.m[4u * y + e]);
                    }
                }
            }
        }
        a.k = (int)kp;
        a.maxQPower = maxQPower;
        HipProfScope prof("mtrx_1q_batch_lds", stream);
        launchMtrx1qBatchLds<R>(wState(), a, stream);
        i += k;
    }
    size_t i = 0;
    while (i < high.size()) {
        const size_t k = std::min(maxK, high.size() - i);
        if (k == 1u) {
            this->Mtrx(&mtrxs[4u * high[i]], targets[high[i]]);
            ++i;
            continue;
        }
        std::vector<size_t> ord(high.begin() + i, high.begin() + i + k);
        std::sort(ord.begin(), ord.end(),
            [&](size_t a, size_t b) { return targets[a] < targets[b]; });
        Batch1qArgs<R> a{};
        for (size_t g = 0; g < k; ++g) {
            a.tPow[g] = pow2(targets[ord[g]]);
            for (int e = 0; e < 4; ++e) a.m[4u * g + e] = mtrxs[4u * ord[g] + e];
        }
        a.k = (int)k;
        a.maxI = maxQPower >> k;
        HipProfScope prof("mtrx_1q_batch", stream);
        launchMtrx1qBatch<R>(wState(), a, stream);
        i += k;
    }
}

template <typename R> void QEngineHIP<R>::XMask(bitCapInt mask)
{
    if (!mask) return;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchXMask<R>(wState(), maxQPower, mask, stream);
}

template <typename R> void QEngineHIP<R>::ZMask(bitCapInt mask)
{
    if (!mask) return;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchParityPhase<R>(wState(), maxQPower, mask, cplx<R>(1, 0), cplx<R>(-1, 0), stream);
}

template <typename R> void QEngineHIP<R>::PhaseParity(R radians, bitCapInt mask)
{
    if (!mask) return;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchParityPhase<R>(
        wState(), maxQPower, mask, polar<R>(1, -radians / 2), polar<R>(1, radians / 2), stream);
}

template <typename R>
void QEngineHIP<R>::UniformlyControlledSingleBit(
    const std::vector<bitLenInt>& controls, bitLenInt target, const cplx<R>* mtrxs)
{
    if (controls.empty()) {
        this->Mtrx(mtrxs, target);
        return;
    }
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const bitCapInt nMtrx = pow2((bitLenInt)controls.size());
    // control powers first, then the matrices, in one upload
    const size_t powBytes = (sizeof(bitCapInt) * controls.size() + 15u) & ~(size_t)15u;
    const size_t mtrxBytes = sizeof(cplx<R>) * 4 * nMtrx;
    QA_HIP_CHECK(hipStreamSynchronize(stream)); // hAux_ and dAux_ are free again
    hAux_.assign(powBytes + mtrxBytes, 0);
    bitCapInt* hPowers = reinterpret_cast<bitCapInt*>(hAux_.data());
    for (size_t i = 0; i < controls.size(); ++i) hPowers[i] = pow2(controls[i]);
    std::memcpy(hAux_.data() + powBytes, mtrxs, mtrxBytes);
    unsigned char* dAux = uploadAux(powBytes + mtrxBytes);
    launchUniformlyControlled<R>(wState(), maxQPower >> 1u, pow2(target),
        reinterpret_cast<const bitCapInt*>(dAux), (int)controls.size(),
        reinterpret_cast<const cplx<R>*>(dAux + powBytes), stream);
}

template <typename R>
void QEngineHIP<R>::PhaseRamp(R scale, bitLenInt rampStart, bitLenInt rampBits, bitCapInt condPower)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("phase_ramp", stream);
    launchPhaseRamp<R>(wState(), maxQPower, rampStart, rampBits, condPower, (double)scale, stream);
}

template <typename R>
void QEngineHIP<R>::QftColumnGeneral(bitLenInt target, double scale, bitLenInt rampStart,
    bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
    const std::vector<uint64_t>& sWeights, double phase0, bool pre)
{
    if (sPows.size() > 8u) throw QrackError("QftColumnGeneral: more than 8 relocated bits");
    RampArgs a{};
    a.rampStart = rampStart;
    a.inPlaceRelMask = inPlaceRelMask;
    a.nScattered = (int)sPows.size();
    for (size_t k = 0; k < sPows.size(); ++k) {
        a.sPow[k] = sPows[k];
        a.sWeight[k] = sWeights[k];
    }
    a.condPow = 0;
    a.scale = scale;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("qft_column", stream);
    launchQftColumnGeneral<R>(wState(), maxQPower, pow2(target), a, phase0, pre, stream);
}

template <typename R>
void QEngineHIP<R>::QftColumn2General(bitLenInt targetHi, bitLenInt targetLo, double scale,
    bitLenInt rampStart, bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
    const std::vector<uint64_t>& sWeights, double phase0Hi, double phase0Lo, bool pre)
{
    if (sPows.size() > 8u) throw QrackError("QftColumn2General: more than 8 relocated bits");
    RampArgs a{};
    a.rampStart = rampStart;
    a.inPlaceRelMask = inPlaceRelMask;
    a.nScattered = (int)sPows.size();
    for (size_t k = 0; k < sPows.size(); ++k) {
        a.sPow[k] = sPows[k];
        a.sWeight[k] = sWeights[k];
    }
    a.condPow = 0;
    a.scale = scale;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("qft_column2_gen", stream);
    launchQftColumn2General<R>(
        wState(), maxQPower, pow2(targetHi), pow2(targetLo), a, phase0Hi, phase0Lo, pre, stream);
}

template <typename R>
void QEngineHIP<R>::QftColumnTopRange(double scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
    const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights, double phase0,
    bool pre, uint64_t itLo, uint64_t itHi, uintptr_t recvPtr, bool recvIsLow, uintptr_t extStream)
{
    if (sPows.size() > 8u) throw QrackError("QftColumnTopRange: more than 8 relocated bits");
    if (!recvPtr) throw QrackError("QftColumnTopRange: null receive buffer");
    RampArgs a{};
    a.rampStart = rampStart;
    a.inPlaceRelMask = inPlaceRelMask;
    a.nScattered = (int)sPows.size();
    for (size_t k = 0; k < sPows.size(); ++k) {
        a.sPow[k] = sPows[k];
        a.sWeight[k] = sWeights[k];
    }
    a.condPow = 0;
    a.scale = scale;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    hipStream_t st = extStream ? (hipStream_t)extStream : stream;
    // a pending basis state is filled on the engine's stream: it must have
    // landed before a kernel on the caller's stream touches the buffer
    const bool wasPending = basisPending_;
    cplx<R>* sv = wState();
    if (wasPending && st != stream) Finish();
    launchQftColumnTopRange<R>(sv, maxQPower, a, phase0, pre, (bitCapInt)itLo, (bitCapInt)itHi,
        (const cplx<R>*)recvPtr, recvIsLow, st);
}

template <typename R>
void QEngineHIP<R>::PhaseRampGeneral(R scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
    const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights, bitCapInt condPower)
{
    if (sPows.size() > 8u) {
        QEngine<R>::PhaseRampGeneral(scale, rampStart, inPlaceRelMask, sPows, sWeights, condPower);
        return;
    }
    QA_HIP_CHECK(hipSetDevice(deviceId));
    RampArgs a{};
    a.rampStart = rampStart;
    a.inPlaceRelMask = inPlaceRelMask;
    a.nScattered = (int)sPows.size();
    for (size_t k = 0; k < sPows.size(); ++k) {
        a.sPow[k] = sPows[k];
        a.sWeight[k] = sWeights[k];
    }
    a.condPow = condPower;
    a.scale = (double)scale;
    HipProfScope prof("phase_ramp", stream);
    launchPhaseRampGeneral<R>(wState(), maxQPower, a, stream);
}

// environment switches of the QFT schedule, read once per process
static const QftPlanOpts& qftPlanOpts()
{
    static const QftPlanOpts opts = []() {
        QftPlanOpts o;
        if (const char* env = std::getenv("QRACK_GPU_QFT_FUSE2")) {
            o.fuseMax = std::atoi(env) != 0 ? 3 : 1;
        } else if (const char* env = std::getenv("QRACK_GPU_QFT_FUSE")) {
            o.fuseMax = std::atoi(env);
        }
        if (const char* env = std::getenv("QRACK_GPU_QFT_LDS")) o.ldsLow = std::atoi(env) != 0;
        // fp64 mid groups would need tiles twice the size; the K4 fusion
        // path serves fp64 there, so the planner keeps mid-LDS fp32-only
        if (const char* env = std::getenv("QRACK_GPU_QFT_MIDLDS")) o.ldsMid = std::atoi(env) != 0;
        // most columns in one mid pass: 9 and 8 allow the wide-tile kernel,
        // 7 and below leave the six-at-a-time schedule
        if (const char* env = std::getenv("QRACK_GPU_QFT_MIDMAX")) o.midMax = std::atoi(env);
        // contiguous-run bits of the wide tile (4 or 5)
        if (const char* env = std::getenv("QRACK_GPU_QFT_WIDELB")) {
            o.wideLowBits = std::atoi(env) == 5 ? 5 : 4;
        }
        return o;
    }();
    return opts;
}

// QRACK_GPU_QFT_SUPPORT=0: a transform of a pending basis state synthesises
// only its first pass and sweeps the whole state in every pass
static bool qaQftSupport()
{
    static const bool v = qaEnvSwitch("QRACK_GPU_QFT_SUPPORT");
    return v;
}

// QRACK_GPU_QFT_SPARSELAST=0: the forward last low pass of such a transform
// runs every orbit of every tile, zeros included
static bool qaQftSparseLast()
{
    static const bool v = qaEnvSwitch("QRACK_GPU_QFT_SPARSELAST");
    return v;
}

template <typename R>
bool QEngineHIP<R>::qftFromBasis(const std::vector<QftPass>& plan, bool inverse, int wideLowBits)
{
    // The state is basisPhase_·|basisPerm_> and stays a product state under
    // every column, so each pass but the last runs only the tiles that can
    // hold a nonzero amplitude and reads the buffer only inside that support
    // (qft_plan.hpp). All passes are enqueued here with no rState()/wState()
    // in between: those would materialise the basis state over the buffer.
    // basisPending_ is dropped after the last enqueue, so a throw on the way
    // leaves the engine pending and correct.
    if constexpr (sizeof(R) == 4) {
        if (!basisPending_ || !qaQftSupport()) return false;
        const QftSupportPlan sp = qftSupportPlan(plan, (int)qubitCount, 0, (int)qubitCount,
            (int)sizeof(R), (unsigned long long)basisPerm_, inverse, wideLowBits);
        if (!sp.eligible) return false;
        const int tb = qaLdsTileBits<R>();
        const int sign = inverse ? -1 : +1;
        bool sumsLeft = false;
        for (size_t k = 0; k < sp.passes.size(); ++k) {
            const QftSupportPass& s = sp.passes[k];
            QftSupportArgs a{};
            a.perm = basisPerm_;
            a.fixedMask = (bitCapInt)s.fixedMask;
            a.tileFree = (bitCapInt)s.tileFree;
            a.tileFixed = (bitCapInt)s.tileFixed;
            a.activeTiles = (bitCapInt)s.activeTiles;
            a.fromBuffer = s.fromBuffer ? 1 : 0;
            if (s.pass.kind == QftPassKind::Low) {
                HipProfScope prof("qft_low_lds", stream);
                // a forward last pass leaves the per-tile norms, under the
                // condition of the unrestricted path
                double* sums = nullptr;
                if (!inverse && k + 1 == sp.passes.size() && tileSumsUsable()
                    && maxQPower >= (ONE_BCI << (tb + 11))) {
                    sums = tileSumsBuffer();
                    sumsLeft = true;
                }
                const bool last = k + 1 == sp.passes.size();
                if (!inverse && last && (s.pass.nCols == 8 || s.pass.nCols == 12)
                    && qaQftSparseLast()) {
                    // only the orbits that hold a nonzero (kernels.hpp)
                    launchQftLowSparseLast(dState_, maxQPower, tb, s.pass.colLo + s.pass.nCols - 1,
                        a, basisPhase_, qftZeroTemplate(s.pass.nCols), sums, stream);
                } else {
                    launchQftLowLdsSupport(dState_, maxQPower, tb,
                        s.pass.colLo + s.pass.nCols - 1, sign, inverse, a, basisPhase_, sums,
                        stream);
                }
            } else {
                HipProfScope prof("qft_mid_lds", stream);
                launchQftMidSupport(dState_, maxQPower, s.lowBits, s.pass.colLo, s.pass.nCols, sign,
                    inverse, a, basisPhase_, stream);
            }
        }
        basisPending_ = false;
        tileSumsValid_ = sumsLeft;
        return true;
    } else {
        (void)plan;
        (void)inverse;
        (void)wideLowBits;
        return false;
    }
}

template <typename R> void QEngineHIP<R>::QFT(bitLenInt start, bitLenInt length, bool)
{
    // Walks the planner's pass list (qft_plan.hpp) top column first. Every
    // pass is one trip over the state: a low ladder or mid pass through LDS
    // tiles, or up to five columns fused in registers, each applying H and
    // the columns' entire controlled-phase ladders
    // (exp(i*pi*(x mod 2^i)/2^i) on the H output's bit-set half).
    if (!length) return;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const QftPlanOpts& opts = qftPlanOpts();
    const int tb = qaLdsTileBits<R>();
    const std::vector<QftPass> plan =
        qftPassPlan((int)length, (int)start, (int)qubitCount, (int)sizeof(R), opts);
    if (basisPending_ && !start && length == qubitCount && qftFromBasis(plan, false, opts.wideLowBits)) {
        return;
    }
    for (const QftPass& p : plan) {
        const bitLenInt lo = (bitLenInt)p.colLo;
        const bitLenInt col = (bitLenInt)(p.colLo + p.nCols - 1);
        if (p.kind == QftPassKind::Low) {
            // the whole remaining (K-aligned) ladder in ONE LDS pass of
            // uniform register-orbit groups
            HipProfScope prof("qft_low_lds", stream);
            if (basisPending_) {
                // first pass from a pending basis state: write-only
                launchQftLowLdsBasis<R>(wStateAll(), maxQPower, tb, (int)col, +1, false,
                    basisPerm_, basisPhase_, stream);
            } else if (tileSumsUsable() && maxQPower >= (ONE_BCI << (tb + 11))) {
                // final pass: leave per-tile norms for the sampler (used
                // once a sampling chunk spans at least one tile)
                double* sums = tileSumsBuffer();
                launchQftLowLdsSums<R>(wState(), maxQPower, tb, (int)col, sums, stream);
                tileSumsValid_ = true;
            } else {
                launchQftLowLds<R>(wState(), maxQPower, tb, (int)col, +1, false, stream);
            }
        } else if (p.kind == QftPassKind::Mid) {
            HipProfScope prof("qft_mid_lds", stream);
            if (p.nCols >= QA_QFT_WIDE_MIN_COLS) {
                if constexpr (sizeof(R) == 4) {
                    const bool basis = basisPending_;
                    cplx<R>* sv = basis ? wStateAll() : wState();
                    launchQftMidWide(sv, maxQPower, opts.wideLowBits, p.colLo, p.nCols, +1, false,
                        basis, basisPerm_, basisPhase_, stream);
                } else {
                    throw QrackError("QFT: wide mid pass planned for a non-fp32 engine");
                }
            } else if (basisPending_) {
                launchQftMidLdsBasis<R>(wStateAll(), maxQPower, p.colLo, p.nCols, +1, false,
                    basisPerm_, basisPhase_, stream);
            } else {
                launchQftMidLds<R>(wState(), maxQPower, p.colLo, p.nCols, +1, false, stream);
            }
        } else if (p.nCols == 5) {
            HipProfScope prof("qft_column5", stream);
            const bitCapInt tPows[5] = { pow2(start + lo), pow2(start + lo + 1u),
                pow2(start + lo + 2u), pow2(start + lo + 3u), pow2(start + lo + 4u) };
            launchQftColumnK<R>(wState(), maxQPower, start, col, 5, tPows, +1, false, stream);
        } else if (p.nCols == 4) {
            HipProfScope prof("qft_column4", stream);
            const bitCapInt tPows[5] = { pow2(start + lo), pow2(start + lo + 1u),
                pow2(start + lo + 2u), pow2(start + lo + 3u), 0u };
            launchQftColumnK<R>(wState(), maxQPower, start, col, 4, tPows, +1, false, stream);
        } else if (p.nCols == 3) {
            // three columns per pass (8-amplitude orbits)
            HipProfScope prof("qft_column3", stream);
            launchQftColumn3<R>(wState(), maxQPower, start, col, pow2(start + col),
                pow2(start + col - 1u), pow2(start + col - 2u), +1, false, stream);
        } else if (p.nCols == 2) {
            HipProfScope prof("qft_column2", stream);
            launchQftColumn2<R>(wState(), maxQPower, start, col, pow2(start + col),
                pow2(start + col - 1u), +1, false, stream);
        } else if (!col) {
            this->H(start);
        } else {
            HipProfScope prof("qft_column", stream);
            launchQftColumn<R>(wState(), maxQPower, start, col, pow2(start + col), +1, false, stream);
        }
    }
}

template <typename R> void QEngineHIP<R>::IQFT(bitLenInt start, bitLenInt length, bool)
{
    // The forward plan walked backwards, lowest pass first, every pass the
    // adjoint (pre-ramp, opposite sign) of the forward one: the exact
    // adjoint schedule whatever the planner chose.
    if (!length) return;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const QftPlanOpts& opts = qftPlanOpts();
    const int tb = qaLdsTileBits<R>();
    const std::vector<QftPass> plan =
        qftPassPlan((int)length, (int)start, (int)qubitCount, (int)sizeof(R), opts);
    if (basisPending_ && !start && length == qubitCount && qftFromBasis(plan, true, opts.wideLowBits)) {
        return;
    }
    for (auto it = plan.rbegin(); it != plan.rend(); ++it) {
        const QftPass& p = *it;
        const bitLenInt lo = (bitLenInt)p.colLo;
        const bitLenInt col = (bitLenInt)(p.colLo + p.nCols - 1);
        if (p.kind == QftPassKind::Low) {
            HipProfScope prof("qft_low_lds", stream);
            if (basisPending_) {
                launchQftLowLdsBasis<R>(wStateAll(), maxQPower, tb, (int)col, -1, true,
                    basisPerm_, basisPhase_, stream);
            } else {
                launchQftLowLds<R>(wState(), maxQPower, tb, (int)col, -1, true, stream);
            }
        } else if (p.kind == QftPassKind::Mid) {
            HipProfScope prof("qft_mid_lds", stream);
            if (p.nCols >= QA_QFT_WIDE_MIN_COLS) {
                if constexpr (sizeof(R) == 4) {
                    const bool basis = basisPending_;
                    cplx<R>* sv = basis ? wStateAll() : wState();
                    launchQftMidWide(sv, maxQPower, opts.wideLowBits, p.colLo, p.nCols, -1, true,
                        basis, basisPerm_, basisPhase_, stream);
                } else {
                    throw QrackError("IQFT: wide mid pass planned for a non-fp32 engine");
                }
            } else if (basisPending_) {
                launchQftMidLdsBasis<R>(wStateAll(), maxQPower, p.colLo, p.nCols, -1, true,
                    basisPerm_, basisPhase_, stream);
            } else {
                launchQftMidLds<R>(wState(), maxQPower, p.colLo, p.nCols, -1, true, stream);
            }
        } else if (p.nCols == 5) {
            HipProfScope prof("qft_column5", stream);
            const bitCapInt tPows[5] = { pow2(start + lo), pow2(start + lo + 1u),
                pow2(start + lo + 2u), pow2(start + lo + 3u), pow2(start + lo + 4u) };
            launchQftColumnK<R>(wState(), maxQPower, start, col, 5, tPows, -1, true, stream);
        } else if (p.nCols == 4) {
            HipProfScope prof("qft_column4", stream);
            const bitCapInt tPows[5] = { pow2(start + lo), pow2(start + lo + 1u),
                pow2(start + lo + 2u), pow2(start + lo + 3u), 0u };
            launchQftColumnK<R>(wState(), maxQPower, start, col, 4, tPows, -1, true, stream);
        } else if (p.nCols == 3) {
            // triple (lo, lo+1, lo+2): exact adjoint of the forward triple
            // (a lo column of 0 degenerates to the plain H inside)
            HipProfScope prof("qft_column3", stream);
            launchQftColumn3<R>(wState(), maxQPower, start, col, pow2(start + col),
                pow2(start + col - 1u), pow2(start + lo), -1, true, stream);
        } else if (p.nCols == 2) {
            HipProfScope prof("qft_column2", stream);
            launchQftColumn2<R>(wState(), maxQPower, start, col, pow2(start + col), pow2(start + lo),
                -1, true, stream);
        } else if (!col) {
            this->H(start);
        } else {
            HipProfScope prof("qft_column", stream);
            launchQftColumn<R>(wState(), maxQPower, start, col, pow2(start + col), -1, true, stream);
        }
    }
}

// ---- reductions -------------------------------------------------------------

template <typename R> double QEngineHIP<R>::reduceSum(int op, const ReduceArgs& a)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("reduce", stream);
    const int grid = launchReduce<R>(rState(), a, op, dPartials, stream);
    QA_HIP_CHECK(hipMemcpyAsync(
        hPartials.data(), dPartials, grid * sizeof(double), hipMemcpyDeviceToHost, stream));
    Finish();
    // compensated sum: up to QA_REDUCE_MAX_BLOCKS partials, and a plain
    // accumulation of that many drifts by several eps of an fp64 result
    double s = 0, comp = 0;
    for (int i = 0; i < grid; ++i) {
        const double y = hPartials[i] - comp;
        const double t = s + y;
        comp = (t - s) - y;
        s = t;
    }
    return s;
}

// ---- Pauli strings and sums -------------------------------------------------

// One launch per (group, chunk of QA_PAULI_MAX_TERMS terms), groups in order
static std::vector<PauliArgs> pauliChunkLaunches(const std::vector<PauliGroup>& groups, bitCapInt nAmps)
{
    std::vector<PauliArgs> launches;
    for (const PauliGroup& g : groups) {
        size_t r = 0, m = 0;
        while (r < g.re.size() || m < g.im.size()) {
            PauliArgs a{};
            a.x = g.x;
            a.nAmps = nAmps;
            while (a.nTerms < QA_PAULI_MAX_TERMS && r < g.re.size()) {
                a.z[a.nTerms] = g.re[r].z;
                a.w[a.nTerms++] = g.re[r++].w;
            }
            a.nRe = a.nTerms;
            while (a.nTerms < QA_PAULI_MAX_TERMS && m < g.im.size()) {
                a.z[a.nTerms] = g.im[m].z;
                a.w[a.nTerms++] = g.im[m++].w;
            }
            launches.push_back(a);
        }
    }
    return launches;
}

template <typename R> double QEngineHIP<R>::pauliGroupsSum(const std::vector<PauliGroup>& groups)
{
    // Each launch folds its block partials (first half of dPartials) into one
    // double in the second half; the whole call's results come back in one copy.
    const std::vector<PauliArgs> launches = pauliChunkLaunches(groups, maxQPower);
    if (launches.empty()) return 0.0;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("pauli", stream);
    const cplx<R>* sv = rState();
    double* dResults = dPartials + QA_REDUCE_MAX_BLOCKS;
    double* hResults = hPartials.data() + QA_REDUCE_MAX_BLOCKS;
    double total = 0;
    for (size_t base = 0; base < launches.size(); base += QA_REDUCE_MAX_BLOCKS) {
        const size_t n = std::min<size_t>(QA_REDUCE_MAX_BLOCKS, launches.size() - base);
        for (size_t k = 0; k < n; ++k) {
            launchPauliGroup<R>(sv, launches[base + k], dPartials, dResults + k, stream);
        }
        QA_HIP_CHECK(hipMemcpyAsync(
            hResults, dResults, n * sizeof(double), hipMemcpyDeviceToHost, stream));
        Finish();
        for (size_t k = 0; k < n; ++k) total += hResults[k];
    }
    return total;
}

template <typename R>
bool QEngineHIP<R>::pauliStringNative(const std::vector<bitLenInt>& bits,
    const std::vector<Pauli>& paulis, const char* what, double& value)
{
    if (bits.size() != paulis.size()) throw QrackError(std::string(what) + ": size mismatch");
    bitCapInt x, z;
    // a repeated or out-of-range qubit keeps the generic lowering's behaviour
    if (!pauliStringMasks(bits, paulis, qubitCount, x, z)) return false;
    if (!x) {
        value = 1.0 - 2.0 * (double)ProbParity(z);
        return true;
    }
    value = pauliGroupsSum({ pauliStringGroup(x, z, 1.0) });
    return true;
}

template <typename R>
double QEngineHIP<R>::PauliExpectation(
    const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis)
{
    double e;
    if (pauliStringNative(bits, paulis, "PauliExpectation", e)) return e;
    return QInterface<R>::PauliExpectation(bits, paulis);
}

template <typename R>
double QEngineHIP<R>::ExpectationPauliAll(
    const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis)
{
    double e;
    if (pauliStringNative(bits, paulis, "ExpectationPauliAll", e)) return e;
    return QInterface<R>::ExpectationPauliAll(bits, paulis);
}

template <typename R>
double QEngineHIP<R>::VariancePauliAll(
    const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis)
{
    double e;
    // the product observable squares to the identity
    if (pauliStringNative(bits, paulis, "VariancePauliAll", e)) return 1.0 - e * e;
    return QInterface<R>::VariancePauliAll(bits, paulis);
}

template <typename R> double QEngineHIP<R>::ExpectationPauliSum(const std::vector<PauliTerm>& terms)
{
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount);
    return c.identity + pauliGroupsSum(c.groups);
}

// ---- reduced density matrices --------------------------------------------------

template <typename R>
void QEngineHIP<R>::GetReducedDensityMatrix(const std::vector<bitLenInt>& qubits, cplx<double>* out)
{
    validateRdmQubits(qubits, qubitCount);
    const int k = (int)qubits.size();
    const size_t D = (size_t)1 << k;
    if (basisPending_) {
        // |perm><perm|: one diagonal entry, nothing to launch
        std::fill(out, out + D * D, cplx<double>(0.0, 0.0));
        size_t a = 0;
        for (int j = 0; j < k; ++j) a |= (size_t)((basisPerm_ >> qubits[j]) & 1u) << j;
        out[a * D + a] = cplx<double>(1.0, 0.0);
        return;
    }
    const RdmPlan plan
        = rdmPassPlan(qubitCount, std::vector<int>(qubits.begin(), qubits.end()), (int)sizeof(R));
    // the kernels index the kept qubits in ascending order: caller index of
    // every such index
    std::vector<int> sorted(plan.tileBits);
    sorted.insert(sorted.end(), plan.blockBits.begin(), plan.blockBits.end());
    std::vector<uint32_t> cidx(D, 0);
    for (int r = 0; r < k; ++r) {
        const int j = (int)(std::find(qubits.begin(), qubits.end(), (bitLenInt)sorted[r]) - qubits.begin());
        for (size_t s = 0; s < D; ++s) {
            if ((s >> r) & 1u) cidx[s] |= 1u << j;
        }
    }
    auto put = [&](size_t sa, size_t sb, double re, double im) {
        const size_t ca = cidx[sa], cb = cidx[sb];
        out[ca * D + cb] = cplx<double>(re, im);
        out[cb * D + ca] = cplx<double>(re, -im);
    };
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("rdm", stream);
    const cplx<R>* sv = rState();

    if (plan.regime == RdmRegime::Register) {
        RdmRegArgs a{};
        for (int r = 0; r < k; ++r) a.pows[r] = pow2((bitLenInt)sorted[r]);
        for (size_t s = 0; s < D; ++s) {
            for (int r = 0; r < k; ++r) {
                if ((s >> r) & 1u) a.off[s] |= a.pows[r];
            }
        }
        const bool keepsBit0 = sorted[0] == 0;
        a.nItems = maxQPower >> k;
        // fp32 with qubit 0 in the environment: an item is a pair of rows
        if (sizeof(R) == 4 && !keepsBit0) a.nItems >>= 1u;
        const size_t nE = D * D;
        const size_t grid = (size_t)rdmRegGrid(a.nItems);
        double* buf = rdmBuffer((grid + 1u) * nE);
        launchRdmReg<R>(sv, k, keepsBit0, a, buf, buf + grid * nE, stream);
        std::vector<double> h(nE);
        QA_HIP_CHECK(hipMemcpyAsync(
            h.data(), buf + grid * nE, nE * sizeof(double), hipMemcpyDeviceToHost, stream));
        Finish();
        for (size_t sa = 0; sa < D; ++sa) {
            put(sa, sa, h[sa * D + sa], 0.0);
            for (size_t sb = sa + 1; sb < D; ++sb) put(sa, sb, h[sa * D + sb], h[sb * D + sa]);
        }
        return;
    }

    const int kt = (int)plan.tileBits.size();
    bitCapInt tileKept = 0, keptAll = 0;
    for (int q : plan.tileBits) tileKept |= pow2((bitLenInt)q);
    for (int q : sorted) keptAll |= pow2((bitLenInt)q);
    std::vector<bitLenInt> env;
    for (bitLenInt q = 0; q < qubitCount; ++q) {
        if (!(keptAll & pow2(q))) env.push_back(q);
    }
    auto makeArgs = [&](int T, bool cross) {
        RdmTileArgs a{};
        const size_t nLow = (size_t)(T - kt); // environment bits inside the tile
        a.tileMask = tileKept;
        for (size_t i = 0; i < env.size(); ++i) (i < nLow ? a.tileMask : a.enumMask) |= pow2(env[i]);
        a.nTiles = ONE_BCI << (env.size() - nLow);
        a.tileAddrBits = T;
        a.cross = cross ? 1 : 0;
        // a block of 256 threads covers 2^LB tile indices per trip
        const int LB = sizeof(R) == 4 ? 9 : 8;
        int pos = 0;
        for (bitLenInt q = 0; q < qubitCount; ++q) {
            if (!(a.tileMask & pow2(q))) continue;
            if (tileKept & pow2(q)) a.keptInTile |= 1u << pos;
            if (pos >= LB) a.tileMaskHigh |= pow2(q);
            ++pos;
        }
        return a;
    };
    const RdmTileArgs diagArgs = makeArgs(plan.tileAddrBits, false);
    const RdmTileArgs crossArgs = makeArgs(plan.crossAddrBits, true);
    auto blockOff = [&](uint32_t v) {
        bitCapInt o = 0;
        for (size_t r = 0; r < plan.blockBits.size(); ++r) {
            if ((v >> r) & 1u) o |= pow2((bitLenInt)plan.blockBits[r]);
        }
        return o;
    };
    const size_t DT = (size_t)1 << kt;
    const size_t NP = DT / 4u;
    const size_t nE = 2u * DT * DT; // stride of a result set; a diagonal launch fills less
    const size_t grid = (size_t)std::max(rdmTileGrid(diagArgs.nTiles), rdmTileGrid(crossArgs.nTiles));
    // results come back in batches: one copy and one sync up to 256 launches
    const size_t batch = std::min<size_t>(plan.launches.size(), 256u);
    double* buf = rdmBuffer((grid + batch) * nE);
    double* results = buf + grid * nE;
    std::vector<double> h(batch * nE);
    for (size_t base = 0; base < plan.launches.size(); base += batch) {
        const size_t n = std::min(batch, plan.launches.size() - base);
        for (size_t l = 0; l < n; ++l) {
            const RdmLaunch& L = plan.launches[base + l];
            RdmTileArgs a = (L.a == L.b) ? diagArgs : crossArgs;
            a.rowOff = blockOff(L.a);
            a.colOff = blockOff(L.b);
            launchRdmTile<R>(sv, kt, a, buf, results + l * nE, stream);
        }
        QA_HIP_CHECK(hipMemcpyAsync(
            h.data(), results, n * nE * sizeof(double), hipMemcpyDeviceToHost, stream));
        Finish();
        for (size_t l = 0; l < n; ++l) {
            const RdmLaunch& L = plan.launches[base + l];
            const double* hl = h.data() + l * nE;
            const bool diag = L.a == L.b;
            const size_t P = (size_t)rdmTilePatches(kt, diag);
            // a diagonal launch numbers the patches pa <= pb row by row, and
            // the block is mirrored from its upper triangle
            size_t pa = 0, pb = 0;
            for (size_t p = 0; p < P; ++p) {
                for (size_t ij = 0; ij < 16u; ++ij) {
                    const size_t ta = pa * 4u + ij / 4u, tb = pb * 4u + ij % 4u;
                    if (diag && ta > tb) continue;
                    const double re = hl[(ij * 2u) * P + p];
                    const double im = (diag && ta == tb) ? 0.0 : hl[(ij * 2u + 1u) * P + p];
                    put(((size_t)L.a << kt) | ta, ((size_t)L.b << kt) | tb, re, im);
                }
                if (++pb == NP) {
                    ++pa;
                    pb = diag ? pa : 0;
                }
            }
        }
    }
}

template <typename R> void QEngineHIP<R>::GetReducedDensityMatrix(bitLenInt q, cplx<R>* out)
{
    cplx<double> rho[4];
    GetReducedDensityMatrix(std::vector<bitLenInt>{ q }, rho);
    for (int t = 0; t < 4; ++t) out[t] = cplx<R>((R)rho[t].re, (R)rho[t].im);
}

// ---- Pauli rotations and Pauli-sum evolution ---------------------------------

template <typename R>
void QEngineHIP<R>::pauliEvolveRun(const PauliCanonSum& c, const PauliEvolvePlan& plan)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* sv = wState();
    // the identity phase rides on the first launch, or is one scalar multiply
    bool phasePending = plan.phase != 0;
    auto fresh = [&](bitCapInt x) {
        PauliEvolveArgs a{};
        a.x = x;
        a.nAmps = maxQPower;
        if (phasePending) {
            a.hasPhase = 1;
            a.phaseRe = std::cos(plan.phase);
            a.phaseIm = -std::sin(plan.phase);
            phasePending = false;
        }
        return a;
    };
    for (const PauliEvolvePass& pass : plan.passes) {
        const PauliEvolveFlat f = pauliEvolveFlatten(c, pass);
        const bitCapInt x = c.groups[pass.group].x;
        HipProfScope prof("pauli_evolve", stream);
        // A launch takes QA_PAULI_MAX_TERMS entries in QA_PAULI_EVOLVE_MAX_SEGS
        // segments (one for the diagonal kernel). A longer segment continues
        // in the next launch: its set commutes, so the split is exact.
        const int maxSegs = x ? QA_PAULI_EVOLVE_MAX_SEGS : 1;
        PauliEvolveArgs a = fresh(x);
        int n = 0;
        size_t t = 0;
        for (size_t k = 0; k < f.segEnd.size(); ++k) {
            while (t < f.segEnd[k]) {
                if (n == QA_PAULI_MAX_TERMS || a.nSeg == maxSegs) {
                    launchPauliEvolve<R>(sv, a, stream);
                    a = fresh(x);
                    n = 0;
                }
                const int seg = a.nSeg++;
                a.segIm[seg] = f.segIm[k] ? 1 : 0;
                while (t < f.segEnd[k] && n < QA_PAULI_MAX_TERMS) {
                    a.z[n] = f.z[t];
                    a.w[n++] = f.w[t++];
                }
                a.segEnd[seg] = n;
                // a one-term segment: the host's cos / sin of its constant |angle|
                const int first = seg ? a.segEnd[seg - 1] : 0;
                if (n - first == 1) {
                    a.segCos[seg] = std::cos(a.w[first]);
                    a.segSin[seg] = std::sin(a.w[first]);
                }
            }
        }
        launchPauliEvolve<R>(sv, a, stream);
    }
    if (phasePending) {
        // nothing but identities: the diagonal kernel with an empty segment
        PauliEvolveArgs a = fresh(0u);
        a.nSeg = 1;
        launchPauliEvolve<R>(sv, a, stream);
    }
}

template <typename R>
void QEngineHIP<R>::PauliRotation(
    const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis, double theta)
{
    const PauliCanonSum c
        = canonicalizePauliSum({ PauliTerm{ 1.0, bits, paulis } }, qubitCount, "PauliRotation");
    pauliEvolveRun(c, pauliEvolvePlan(c, theta, 1, 1));
}

template <typename R>
void QEngineHIP<R>::EvolvePauliSum(
    const std::vector<PauliTerm>& terms, double time, int steps, int order)
{
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "EvolvePauliSum");
    pauliEvolveRun(c, pauliEvolvePlan(c, time, steps, order));
}

// ---- Pauli brakets, H|psi>, adjoint gradient -----------------------------------

template <typename R> void QEngineHIP<R>::releasePairResults()
{
    if (dPairRes_) hipFree(dPairRes_);
    dPairRes_ = nullptr;
    pairResLen_ = 0;
}

template <typename R> double* QEngineHIP<R>::pairResults(size_t n)
{
    if (n <= pairResLen_) return dPairRes_;
    QA_HIP_CHECK(hipStreamSynchronize(stream)); // nothing still writes the old slots
    releasePairResults();
    QA_HIP_CHECK(hipMalloc(&dPairRes_, 2u * n * sizeof(double)));
    pairResLen_ = n;
    return dPairRes_;
}

namespace {
// the launches of a canonical sum; a sum without non-identity terms is one
// diagonal launch with an empty table
std::vector<PauliArgs> pauliSumLaunches(const PauliCanonSum& c, bitCapInt nAmps)
{
    std::vector<PauliArgs> launches = pauliChunkLaunches(c.groups, nAmps);
    if (launches.empty()) {
        PauliArgs a{};
        a.nAmps = nAmps;
        launches.push_back(a);
    }
    return launches;
}
} // namespace

template <typename R>
cplx<double> QEngineHIP<R>::PauliSumBraket(QInterfacePtr<R> bra, const std::vector<PauliTerm>& terms)
{
    if (bra->GetQubitCount() != qubitCount) throw QrackError("PauliSumBraket: width mismatch");
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "PauliSumBraket");
    const std::vector<PauliArgs> launches = pauliSumLaunches(c, maxQPower);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    // a staged copy of the bra is freed on every way out
    struct Staged {
        QEngineHIP<R>* self;
        cplx<R>* p = nullptr;
        ~Staged() { self->freeDev(p, self->maxQPower); }
    } staged{ this };
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(bra.get());
    const cplx<R>* braBuf = nullptr;
    if (o == this) {
        braBuf = rState();
    } else if (o && o->deviceId == deviceId) {
        braBuf = o->rState();
        o->Finish();
    } else {
        std::vector<cplx<R>> host(maxQPower);
        bra->GetQuantumState(host.data());
        staged.p = allocDev(maxQPower);
        QA_HIP_CHECK(hipMemcpyAsync(
            staged.p, host.data(), sizeof(cplx<R>) * maxQPower, hipMemcpyHostToDevice, stream));
        QA_HIP_CHECK(hipStreamSynchronize(stream)); // host goes out of scope
        braBuf = staged.p;
    }
    const cplx<R>* sv = rState();
    double* dRes = pairResults(launches.size());
    std::vector<double> hRes(2u * launches.size());
    {
        HipProfScope prof("pauli_braket", stream);
        // the identity's share rides on the first launch: both vectors are in hand
        for (size_t k = 0; k < launches.size(); ++k) {
            launchPauliBraket<R>(
                sv, braBuf, launches[k], k ? 0.0 : c.identity, dPartials, dRes + 2u * k, stream);
        }
        QA_HIP_CHECK(hipMemcpyAsync(
            hRes.data(), dRes, hRes.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        Finish();
    }
    double re = 0, im = 0;
    for (size_t k = 0; k < launches.size(); ++k) {
        re += hRes[2u * k];
        im += hRes[2u * k + 1u];
    }
    return cplx<double>(re, im);
}

template <typename R>
void QEngineHIP<R>::pauliApplyRun(const PauliCanonSum& c, const cplx<R>* src, cplx<R>* dst)
{
    const std::vector<PauliArgs> launches = pauliSumLaunches(c, maxQPower);
    for (size_t k = 0; k < launches.size(); ++k) {
        HipProfScope prof("pauli_apply", stream);
        launchPauliApply<R>(src, dst, launches[k], c.identity, k == 0u, stream);
    }
}

template <typename R>
void QEngineHIP<R>::PauliSumApplyInto(const std::vector<PauliTerm>& terms, QInterfacePtr<R> dest)
{
    if (dest.get() == this) throw QrackError("PauliSumApplyInto: dest is this simulator");
    if (dest->GetQubitCount() != qubitCount) throw QrackError("PauliSumApplyInto: width mismatch");
    QEngineHIP<R>* d = dynamic_cast<QEngineHIP<R>*>(dest.get());
    if (!d || d->deviceId != deviceId)
        throw QrackError("PauliSumApplyInto: dest must be a HIP engine on the same device");
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "PauliSumApplyInto");
    QA_HIP_CHECK(hipSetDevice(deviceId));
    d->Finish(); // whatever dest still had queued on its own stream
    const cplx<R>* src = rState();
    pauliApplyRun(c, src, d->wStateAll());
    Finish(); // dest's stream may use the buffer from here on
    d->runningNorm = (R)-1;
}

template <typename R>
void QEngineHIP<R>::pauliRotateBuffer(cplx<R>* buf, const PauliGroup& g, double angle)
{
    const bool isIm = !g.im.empty();
    const PauliCanonTerm t = isIm ? g.im[0] : g.re[0];
    PauliEvolveArgs a{};
    a.x = g.x;
    a.nAmps = maxQPower;
    a.nSeg = 1;
    a.segEnd[0] = 1;
    a.segIm[0] = isIm ? 1 : 0;
    a.z[0] = t.z;
    a.w[0] = angle * t.w;
    a.segCos[0] = std::cos(a.w[0]);
    a.segSin[0] = std::sin(a.w[0]);
    HipProfScope prof("pauli_evolve", stream);
    launchPauliEvolve<R>(buf, a, stream);
}

template <typename R>
double QEngineHIP<R>::AdjointGradient(const std::vector<AdjointOp<R>>& ops,
    const std::vector<PauliTerm>& terms, std::vector<double>& grad)
{
    validateAdjointOps(ops, qubitCount);
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "AdjointGradient");
    grad.clear();
    QA_HIP_CHECK(hipSetDevice(deviceId));
    size_t nTrain = 0;
    for (const AdjointOp<R>& op : ops) {
        if (op.kind == AdjointOp<R>::Rotation && op.trainable) ++nTrain;
    }
    // slot 0: <lambda|psi_N>; slot 1 + t: <lambda|P|psi> of trainable rotation t
    double* dRes = pairResults(nTrain + 1u);
    // the second vector: a raw buffer the allocation cap counts, freed on
    // every way out. Taken before the state is touched, so that a refusal
    // leaves psi_0 in place.
    struct Lambda {
        QEngineHIP<R>* self;
        cplx<R>* p = nullptr;
        ~Lambda() { self->freeDev(p, self->maxQPower); }
    } lam{ this };
    lam.p = allocDev(maxQPower);
    for (const AdjointOp<R>& op : ops) {
        if (op.kind == AdjointOp<R>::Rotation) {
            PauliRotation(op.qubits, op.paulis, op.theta);
        } else {
            MtrxN(op.qubits, op.mtrx.data(), op.controls, op.anti);
        }
    }
    pauliApplyRun(c, wState(), lam.p);
    {
        // E = Re <lambda|psi_N>: the braket of the identity alone
        PauliArgs a{};
        a.nAmps = maxQPower;
        HipProfScope prof("pauli_braket", stream);
        launchPauliBraket<R>(rState(), lam.p, a, 1.0, dPartials, dRes, stream);
    }
    // what a launcher of this engine does to the state, done to lambda
    auto onLambda = [&](const std::function<void()>& f) {
        std::swap(dState_, lam.p);
        try {
            f();
        } catch (...) {
            std::swap(dState_, lam.p);
            throw;
        }
        std::swap(dState_, lam.p);
    };
    size_t slot = nTrain;
    for (size_t k = ops.size(); k-- > 0u;) {
        const AdjointOp<R>& op = ops[k];
        if (op.kind == AdjointOp<R>::Gate) {
            const std::vector<cplx<R>> dag = adjointOpDagger(op);
            MtrxN(op.qubits, dag.data(), op.controls, op.anti);
            onLambda([&] { MtrxN(op.qubits, dag.data(), op.controls, op.anti); });
            continue;
        }
        bitCapInt x, z;
        pauliStringMasks(op.qubits, op.paulis, qubitCount, x, z);
        const PauliGroup g = pauliStringGroup(x, z, 1.0);
        if (!op.trainable) {
            pauliRotateBuffer(wState(), g, -op.theta);
            pauliRotateBuffer(lam.p, g, -op.theta);
            continue;
        }
        const bool isIm = !g.im.empty();
        const PauliCanonTerm t = isIm ? g.im[0] : g.re[0];
        PauliAdjointArgs a{};
        a.x = x;
        a.z = t.z;
        a.nAmps = maxQPower;
        a.im = isIm ? 1 : 0;
        a.w = t.w;
        a.cs = std::cos(-op.theta * t.w);
        a.sn = std::sin(-op.theta * t.w);
        HipProfScope prof("pauli_adjoint", stream);
        launchPauliAdjoint<R>(wState(), lam.p, a, dPartials, dRes + 2u * slot, stream);
        --slot;
    }
    std::vector<double> hRes(2u * (nTrain + 1u));
    QA_HIP_CHECK(hipMemcpyAsync(
        hRes.data(), dRes, hRes.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    Finish();
    grad.resize(nTrain);
    for (size_t t = 0; t < nTrain; ++t) grad[t] = 2.0 * hRes[2u * (t + 1u) + 1u];
    return hRes[0];
}

// ---- Krylov evolution and Lanczos (krylov.hpp) ---------------------------------

static_assert((size_t)QA_PAULI_MAX_TERMS == PAULI_SUM_LAUNCH_TERMS,
    "pauliSumLaunchCount's default chunk is the launch table's size");

template <typename R>
KrylovRun QEngineHIP<R>::lanczosRun(
    const PauliCanonSum& c, int dim, const std::vector<cplx<R>*>& bufs, const char* what)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const std::vector<PauliArgs> launches = pauliSumLaunches(c, maxQPower);
    const size_t L = launches.size();
    ReduceArgs ra{};
    ra.maxI = maxQPower;
    const double nrm = reduceSum((int)ReduceOp::NORM_ALL, ra);
    if (!(nrm > 0)) throw QrackError(std::string(what) + ": the state has zero norm");
    const double theta = krylovTheta(L, (double)std::numeric_limits<R>::epsilon(), pauliSumAbsWeights(c));
    // one slot per launch for its share of alpha, then (alpha's sum, beta^2)
    double* dSlots = pairResults((L + 3u) / 2u);
    double* dRes = dSlots + L;
    const cplx<R>* sv = rState();
    const size_t nb = bufs.size();
    return lanczosDrive(dim, std::sqrt(nrm), theta, [&](int j, double s, double b) {
        const cplx<R>* u = (j == 1) ? sv : bufs[(size_t)(j - 2) % nb];
        const cplx<R>* prev = (j == 1) ? nullptr : (j == 2) ? sv : bufs[(size_t)(j - 3) % nb];
        cplx<R>* dest = bufs[(size_t)(j - 1) % nb];
        for (size_t k = 0; k < L; ++k) {
            // the scale of the unnormalised basis rides in the weights, in double
            PauliArgs a = launches[k];
            for (int t = 0; t < a.nTerms; ++t) a.w[t] *= s;
            HipProfScope prof("krylov_apply", stream);
            launchKrylovApply<R>(u, prev, dest, a, s * c.identity, b, k == 0u, dPartials, dSlots + k, stream);
        }
        double h[2] = { 0, 0 };
        {
            HipProfScope prof("krylov_finish", stream);
            launchKrylovFinish<R>(u, dest, maxQPower, dSlots, (int)L, s * s, j < dim, dPartials, dRes, stream);
            QA_HIP_CHECK(hipMemcpyAsync(h, dRes, sizeof(h), hipMemcpyDeviceToHost, stream));
            Finish(); // the host needs beta for the next scale
        }
        return std::pair<double, double>(h[0], h[1]);
    });
}

template <typename R>
void QEngineHIP<R>::krylovCombine(const std::vector<cplx<double>>& coef, const std::vector<cplx<R>*>& bufs)
{
    cplx<R>* sv = wState();
    const size_t nSrc = coef.size() - 1u;
    size_t done = 0;
    bool first = true;
    do {
        KrylovCombineArgs<R> a{};
        a.coefRe[0] = first ? coef[0].re : 1.0;
        a.coefIm[0] = first ? coef[0].im : 0.0;
        while (a.nSrc < KRYLOV_COMBINE_MAX_VECTORS && done < nSrc) {
            a.src[a.nSrc] = bufs[done];
            a.coefRe[a.nSrc + 1] = coef[done + 1u].re;
            a.coefIm[a.nSrc + 1] = coef[done + 1u].im;
            ++a.nSrc;
            ++done;
        }
        HipProfScope prof("krylov_combine", stream);
        launchKrylovCombine<R>(sv, maxQPower, a, stream);
        first = false;
    } while (done < nSrc);
    Finish(); // the sources are freed by the caller
}

template <typename R>
void QEngineHIP<R>::LanczosTridiagonal(const std::vector<PauliTerm>& terms, int dim,
    std::vector<double>& alpha, std::vector<double>& beta)
{
    validateKrylovArgs(dim, 1, "LanczosTridiagonal");
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "LanczosTridiagonal");
    QA_HIP_CHECK(hipSetDevice(deviceId));
    KrylovBuffers bufs(this);
    bufs.take((size_t)std::min(dim, 3));
    const KrylovRun run = lanczosRun(c, dim, bufs.p, "LanczosTridiagonal");
    alpha = run.alpha;
    beta = run.beta;
}

template <typename R>
double QEngineHIP<R>::KrylovEvolvePauliSum(const std::vector<PauliTerm>& terms, double time, int dim, int steps)
{
    validateKrylovArgs(dim, steps, "KrylovEvolvePauliSum");
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "KrylovEvolvePauliSum");
    if (time == 0) return 0.0;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    KrylovBuffers bufs(this);
    bufs.take((size_t)dim);
    const double tau = time / steps;
    double estimate = 0;
    for (int st = 0; st < steps; ++st) {
        const KrylovRun run = lanczosRun(c, dim, bufs.p, "KrylovEvolvePauliSum");
        std::vector<cplx<double>> coef = krylovCoefficients(run.alpha, run.beta, tau);
        const size_t k = run.k();
        estimate += run.beta[k - 1u]
            * std::sqrt(coef[k - 1u].re * coef[k - 1u].re + coef[k - 1u].im * coef[k - 1u].im);
        for (size_t j = 0; j < k; ++j) coef[j] = (run.norm0 * run.scale[j]) * coef[j];
        krylovCombine(coef, bufs.p);
        runningNorm = (R)-1;
    }
    return estimate;
}

template <typename R>
std::pair<double, double> QEngineHIP<R>::LanczosGroundState(const std::vector<PauliTerm>& terms, int dim, bool prepare)
{
    validateKrylovArgs(dim, 1, "LanczosGroundState");
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "LanczosGroundState");
    QA_HIP_CHECK(hipSetDevice(deviceId));
    KrylovBuffers bufs(this);
    bufs.take((size_t)(prepare ? dim : std::min(dim, 3)));
    const KrylovRun run = lanczosRun(c, dim, bufs.p, "LanczosGroundState");
    std::vector<double> y;
    const double lambda = krylovLowestRitz(run.alpha, run.beta, y);
    const size_t k = run.k();
    if (prepare) {
        std::vector<cplx<double>> coef(k);
        for (size_t j = 0; j < k; ++j) coef[j] = cplx<double>(y[j] * run.scale[j], 0.0);
        krylovCombine(coef, bufs.p);
        // without re-orthogonalisation the basis is orthonormal only until a
        // Ritz pair converges, and the sum's norm is off by as much: one
        // reduction and one scaling pass make "unit norm" hold
        ReduceArgs ra{};
        ra.maxI = maxQPower;
        const double nrm = reduceSum((int)ReduceOp::NORM_ALL, ra);
        if (nrm > 0) {
            launchNormalize<R>(wState(), maxQPower, cplx<R>((R)(1.0 / std::sqrt(nrm)), (R)0), (R)0, stream);
        }
        runningNorm = (R)1;
    }
    return { lambda, run.beta[k - 1u] * std::abs(y[k - 1u]) };
}

template <typename R>
KrylovEigenResult QEngineHIP<R>::LanczosLowestStates(
    const std::vector<PauliTerm>& terms, int nev, int dim, double tol, int maxRestarts, int prepare)
{
    validateKrylovEigenArgs(nev, dim, tol, maxRestarts, prepare);
    const PauliCanonSum c = canonicalizePauliSum(terms, qubitCount, "LanczosLowestStates");
    QA_HIP_CHECK(hipSetDevice(deviceId));
    // the basis and w, all up front: a refusal leaves the state untouched. A
    // cycle after a restart has no state among its dim vectors, hence one more
    KrylovBuffers bufs(this);
    bufs.take((size_t)dim + (maxRestarts > 0 ? 1u : 0u));
    const std::vector<PauliArgs> launches = pauliSumLaunches(c, maxQPower);
    const size_t L = launches.size();
    ReduceArgs ra{};
    ra.maxI = maxQPower;
    const double nrm = reduceSum((int)ReduceOp::NORM_ALL, ra);
    if (!(nrm > 0)) throw QrackError("LanczosLowestStates: the state has zero norm");
    const double theta = krylovTheta(L, (double)std::numeric_limits<R>::epsilon(), pauliSumAbsWeights(c));
    // 33 results for every orth launch of a step, then the slots where the
    // apply launches leave their shares of <u|H u>, which nobody reads. The
    // block partials of a launch go through dPartials, in stream order.
    constexpr size_t Q = (size_t)KRYLOV_ORTH_RESULTS;
    const size_t maxLaunches = (size_t)krylovOrthLaunches(dim);
    double* dOrthRes = pairResults((Q * maxLaunches + L + 1u) / 2u);
    double* dSlots = dOrthRes + Q * maxLaunches;
    double* dOrthPartials = dPartials;
    std::vector<double> hRes(Q * maxLaunches);

    const cplx<R>* sv = rState();
    std::vector<const cplx<R>*> basis(1, sv);
    std::vector<cplx<R>*> spare(bufs.p.rbegin(), bufs.p.rend());
    cplx<R>* w = nullptr;
    constexpr int CAP = KRYLOV_ORTH_MAX_VECTORS;

    auto step = [&](int j, const std::vector<double>& scale) {
        w = spare.back();
        const double s = scale[(size_t)(j - 1)];
        for (size_t k = 0; k < L; ++k) {
            PauliArgs a = launches[k];
            for (int t = 0; t < a.nTerms; ++t) a.w[t] *= s;
            HipProfScope prof("krylov_apply", stream);
            launchKrylovApply<R>(
                basis[(size_t)(j - 1)], nullptr, w, a, s * c.identity, 0.0, k == 0u, dPartials, dSlots + k, stream);
        }
        auto chunk = [&](int g0) {
            KrylovOrthArgs<R> a{};
            a.n = std::min(CAP, j - g0);
            for (int i = 0; i < a.n; ++i) {
                a.u[i] = basis[(size_t)(g0 + i)];
                a.scale[i] = scale[(size_t)(g0 + i)] * scale[(size_t)(g0 + i)];
            }
            return a;
        };
        size_t nLaunch = 0;
        auto orth = [&](const KrylovOrthArgs<R>& a, const double* coef) {
            double* res = dOrthRes + Q * nLaunch++;
            HipProfScope prof("krylov_orth", stream);
            launchKrylovOrth<R>(w, maxQPower, a, coef, coef != nullptr, dOrthPartials, res, stream);
            return res;
        };
        KrylovOrthStep r;
        r.h.assign((size_t)j, cplx<double>(0.0, 0.0));
        // which launch's results hold c_i of (round, chunk)
        std::vector<std::pair<size_t, int>> ips;
        if (j <= CAP) {
            const KrylovOrthArgs<R> a = chunk(0);
            const double* r0 = orth(a, nullptr);
            const double* r1 = orth(a, r0);
            orth(a, r1);
            ips = { { 0u, 0 }, { 1u, 0 } };
        } else {
            for (int round = 0; round < 2; ++round) {
                for (int g0 = 0; g0 < j; g0 += CAP) {
                    const KrylovOrthArgs<R> a = chunk(g0);
                    ips.push_back({ nLaunch, g0 });
                    orth(a, orth(a, nullptr));
                }
            }
        }
        QA_HIP_CHECK(hipMemcpyAsync(
            hRes.data(), dOrthRes, Q * nLaunch * sizeof(double), hipMemcpyDeviceToHost, stream));
        Finish(); // the host needs beta for the next scale
        for (const std::pair<size_t, int>& ip : ips) {
            const double* res = hRes.data() + Q * ip.first;
            const int n = std::min(CAP, j - ip.second);
            for (int i = 0; i < n; ++i) {
                const double si = scale[(size_t)(ip.second + i)];
                cplx<double>& h = r.h[(size_t)(ip.second + i)];
                h = h + cplx<double>(si * res[2 * i], si * res[2 * i + 1]);
            }
        }
        r.norm2 = hRes[Q * (nLaunch - 1u) + Q - 1u];
        return r;
    };
    auto accept = [&]() {
        basis.push_back(w);
        spare.pop_back();
    };
    auto rotate = [&](int k, int kp, const std::vector<double>& m) {
        // the outputs take the place of inputs, never the state's
        std::vector<cplx<R>*> own;
        for (const cplx<R>* b : basis) {
            if (b != sv) own.push_back(const_cast<cplx<R>*>(b));
        }
        KrylovRotateArgs<R> a{};
        a.k = k;
        a.kp = kp;
        for (int r = 0; r < k; ++r) a.in[r] = basis[(size_t)r];
        for (int i = 0; i < kp; ++i) a.out[i] = own[(size_t)i];
        constexpr size_t N = (size_t)KRYLOV_COMBINE_MAX_VECTORS;
        QA_HIP_CHECK(hipStreamSynchronize(stream)); // hAux_ and dAux_ are free again
        hAux_.assign(sizeof(R) * (size_t)k * N, 0);
        R* hm = reinterpret_cast<R*>(hAux_.data());
        for (int r = 0; r < k; ++r) {
            for (int i = 0; i < kp; ++i) hm[(size_t)r * N + (size_t)i] = (R)m[(size_t)r * (size_t)kp + (size_t)i];
        }
        const R* dm = reinterpret_cast<const R*>(uploadAux(hAux_.size()));
        {
            HipProfScope prof("krylov_rotate", stream);
            launchKrylovRotate<R>(a, dm, maxQPower, stream);
        }
        spare.pop_back(); // w, which becomes u~_(kp+1)
        for (size_t i = (size_t)kp; i < own.size(); ++i) spare.push_back(own[i]);
        basis.assign(own.begin(), own.begin() + kp);
        basis.push_back(w);
    };
    const KrylovEigenRun run = krylovEigenDrive(
        nev, dim, tol, maxRestarts, prepare, std::sqrt(nrm), theta, step, accept, rotate);
    if (prepare >= 0) {
        if (run.prepareCoef.empty()) {
            throw QrackError("LanczosLowestStates: the run ended with fewer than prepare + 1 pairs");
        }
        // krylovCombine's form: the state's own coefficient first
        const bool first = basis[0] == sv;
        std::vector<cplx<double>> coef(1, cplx<double>(first ? run.prepareCoef[0] : 0.0, 0.0));
        std::vector<cplx<R>*> src;
        for (size_t r = first ? 1u : 0u; r < basis.size(); ++r) {
            coef.push_back(cplx<double>(run.prepareCoef[r], 0.0));
            src.push_back(const_cast<cplx<R>*>(basis[r]));
        }
        krylovCombine(coef, src);
        runningNorm = (R)1;
    }
    return run.result;
}

template <typename R> std::pair<double, bitCapInt> QEngineHIP<R>::argMax()
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const int grid = launchArgMax<R>(rState(), maxQPower, dPartials, dIdx, stream);
    std::vector<bitCapInt> hIdx(grid);
    QA_HIP_CHECK(hipMemcpyAsync(
        hPartials.data(), dPartials, grid * sizeof(double), hipMemcpyDeviceToHost, stream));
    QA_HIP_CHECK(
        hipMemcpyAsync(hIdx.data(), dIdx, grid * sizeof(bitCapInt), hipMemcpyDeviceToHost, stream));
    Finish();
    int best = 0;
    for (int i = 1; i < grid; ++i) {
        if (hPartials[i] > hPartials[best]) best = i;
    }
    return { hPartials[best], hIdx[best] };
}

template <typename R> R QEngineHIP<R>::Prob(bitLenInt q)
{
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.mask = pow2(q);
    const double p = reduceSum((int)ReduceOp::PROB_BITSET, a);
    return (R)std::min(1.0, std::max(0.0, p));
}

template <typename R> R QEngineHIP<R>::ProbMask(bitCapInt mask, bitCapInt permutation)
{
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.mask = mask;
    a.perm = permutation;
    const double p = reduceSum((int)ReduceOp::PROB_MASK, a);
    return (R)std::min(1.0, std::max(0.0, p));
}

template <typename R> R QEngineHIP<R>::ProbReg(bitLenInt start, bitLenInt length, bitCapInt permutation)
{
    return ProbMask(pow2Mask(length) << start, permutation << start);
}

template <typename R> R QEngineHIP<R>::ProbParity(bitCapInt mask)
{
    if (!mask) return 0;
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.mask = mask;
    const double p = reduceSum((int)ReduceOp::PROB_PARITY, a);
    return (R)std::min(1.0, std::max(0.0, p));
}

template <typename R> bool QEngineHIP<R>::ForceMParity(bitCapInt mask, bool result, bool doForce)
{
    if (!mask) return false;
    const R oddProb = ProbParity(mask);
    if (!doForce) result = (this->Rand() < (double)oddProb);
    const R prob = result ? oddProb : ((R)1 - oddProb);
    if (prob <= 0) throw QrackError("ForceMParity: impossible outcome");
    const R nrm = (R)1 / std::sqrt(prob);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchApplyParity<R>(wState(), maxQPower, mask, result, cplx<R>(nrm, 0), stream);
    runningNorm = (R)1;
    return result;
}

template <typename R> void QEngineHIP<R>::ApplyM(bitCapInt regMask, bitCapInt result, cplx<R> nrm)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchApplyM<R>(wState(), maxQPower, regMask, result, nrm, stream);
    runningNorm = (R)1;
}

template <typename R>
double QEngineHIP<R>::ExpectationBitsFactorized(
    const std::vector<bitLenInt>& bits, const std::vector<bitCapInt>& perms, bitCapInt offset)
{
    if (bits.size() > (size_t)QA_REDUCE_MAX_BITS) {
        return QEngine<R>::ExpectationBitsFactorized(bits, perms, offset);
    }
    QA_HIP_CHECK(hipSetDevice(deviceId));
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.offset = (double)offset;
    for (size_t b = 0; b < bits.size(); ++b) {
        a.bitsArr[b] = bits[b];
        a.permsArr[b] = perms[b];
    }
    a.nBits = (int)bits.size();
    return reduceSum((int)ReduceOp::EXP_PERM, a);
}

template <typename R>
double QEngineHIP<R>::VarianceBitsAll(const std::vector<bitLenInt>& bits, bitCapInt offset)
{
    if (bits.size() > (size_t)QA_REDUCE_MAX_BITS) {
        return QEngine<R>::VarianceBitsAll(bits, offset);
    }
    const double mean = this->ExpectationBitsAll(bits, offset);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.offset = (double)offset;
    for (size_t b = 0; b < bits.size(); ++b) {
        a.bitsArr[b] = bits[b];
        a.permsArr[b] = pow2((bitLenInt)b);
    }
    a.nBits = (int)bits.size();
    const double e2 = reduceSum((int)ReduceOp::EXP_PERM_SQ, a);
    return e2 - mean * mean;
}

// ---- sampling ---------------------------------------------------------------

template <typename R> std::vector<double> QEngineHIP<R>::chunkSums(bitCapInt& chunkLenOut)
{
    const bitCapInt nChunks = std::min<bitCapInt>(maxQPower, 2048u);
    const bitCapInt chunkLen = maxQPower / nChunks;
    chunkLenOut = chunkLen;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const int tb = qaLdsTileBits<R>();
    if (tileSumsValid_ && tileSumsUsable() && dTileSums_ && chunkLen >= (ONE_BCI << tb)) {
        // the last QFT pass left per-tile norms of exactly this state: add
        // them per chunk instead of re-reading the whole state
        launchTileChunkSums(dTileSums_, nChunks, chunkLen >> tb, dPartials, stream);
    } else {
        launchChunkSums<R>(rState(), nChunks, chunkLen, dPartials, stream);
    }
    std::vector<double> sums(nChunks);
    QA_HIP_CHECK(hipMemcpyAsync(
        sums.data(), dPartials, nChunks * sizeof(double), hipMemcpyDeviceToHost, stream));
    Finish();
    return sums;
}

template <typename R>
bitCapInt QEngineHIP<R>::sampleOnce(const std::vector<double>& sums, bitCapInt chunkLen, double r,
    std::vector<cplx<R>>& hostChunk, bitCapInt& cachedChunk)
{
    // r in [0, total)
    bitCapInt c = 0;
    while (c + 1 < (bitCapInt)sums.size() && r > sums[c]) {
        r -= sums[c];
        ++c;
    }
    if (cachedChunk != c) {
        GetAmplitudePage(hostChunk.data(), c * chunkLen, chunkLen);
        cachedChunk = c;
    }
    bitCapInt i = 0;
    for (; i < chunkLen - 1; ++i) {
        r -= (double)norm(hostChunk[i]);
        if (r <= 0) break;
    }
    return c * chunkLen + i;
}

template <typename R> bitCapInt QEngineHIP<R>::MAll()
{
    bitCapInt chunkLen = 0;
    const std::vector<double> sums = chunkSums(chunkLen);
    double total = 0;
    for (double s : sums) total += s;
    std::vector<cplx<R>> hostChunk(chunkLen);
    bitCapInt cached = (bitCapInt)-1;
    const bitCapInt result = sampleOnce(sums, chunkLen, this->Rand() * total, hostChunk, cached);
    SetPermutation(result);
    return result;
}

template <typename R> bitCapInt QEngineHIP<R>::HighestProbAll()
{
    return argMax().second;
}

template <typename R>
std::map<bitCapInt, int> QEngineHIP<R>::MultiShotMeasureMask(
    const std::vector<bitCapInt>& qPowers, unsigned shots)
{
    if (!shots) return {};
    bitCapInt chunkLen = 0;
    const std::vector<double> sums = chunkSums(chunkLen);
    double total = 0;
    for (double s : sums) total += s;
    std::vector<double> rs(shots);
    for (unsigned s = 0; s < shots; ++s) rs[s] = this->Rand() * total;
    std::sort(rs.begin(), rs.end());
    std::vector<cplx<R>> hostChunk(chunkLen);
    bitCapInt cached = (bitCapInt)-1;
    std::map<bitCapInt, int> results;
    for (unsigned s = 0; s < shots; ++s) {
        const bitCapInt i = sampleOnce(sums, chunkLen, rs[s], hostChunk, cached);
        bitCapInt val = 0;
        for (size_t b = 0; b < qPowers.size(); ++b) {
            if (i & qPowers[b]) val |= (ONE_BCI << b);
        }
        results[val]++;
    }
    return results;
}

// ---- norm -------------------------------------------------------------------

template <typename R> void QEngineHIP<R>::UpdateRunningNorm(R norm_thresh)
{
    if (norm_thresh < 0) norm_thresh = amplitudeFloor;
    ReduceArgs a{};
    a.maxI = maxQPower;
    a.normThresh = (double)norm_thresh;
    runningNorm = (R)reduceSum((int)ReduceOp::NORM_FLOOR, a);
}

template <typename R> void QEngineHIP<R>::NormalizeState(R nrm, R norm_thresh, R phaseArg)
{
    if (nrm < 0) {
        if (runningNorm < 0) UpdateRunningNorm(norm_thresh);
        nrm = runningNorm;
    }
    if (nrm <= 0) return;
    if (norm_thresh < 0) norm_thresh = amplitudeFloor;
    const cplx<R> factor = polar<R>((R)(1.0 / std::sqrt((double)nrm)), phaseArg);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchNormalize<R>(wState(), maxQPower, factor, norm_thresh * nrm, stream);
    runningNorm = (R)1;
}

template <typename R> double QEngineHIP<R>::SumSqrDiff(QInterfacePtr<R> other)
{
    if (other->GetQubitCount() != qubitCount) return 2.0;
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(other.get());
    QA_HIP_CHECK(hipSetDevice(deviceId));
    const cplx<R>* otherBuf = nullptr;
    cplx<R>* tmp = nullptr;
    if (o && o->deviceId == deviceId) {
        otherBuf = o->rState();
        o->Finish();
    } else {
        std::vector<cplx<R>> host(maxQPower);
        other->GetQuantumState(host.data());
        tmp = allocDev(maxQPower);
        QA_HIP_CHECK(hipMemcpyAsync(
            tmp, host.data(), sizeof(cplx<R>) * maxQPower, hipMemcpyHostToDevice, stream));
        otherBuf = tmp;
    }
    const int grid = launchInner<R>(
        rState(), otherBuf, maxQPower, dPartials, dPartials + QA_REDUCE_MAX_BLOCKS, stream);
    QA_HIP_CHECK(hipMemcpyAsync(
        hPartials.data(), dPartials, grid * sizeof(double), hipMemcpyDeviceToHost, stream));
    QA_HIP_CHECK(hipMemcpyAsync(hPartials.data() + QA_REDUCE_MAX_BLOCKS,
        dPartials + QA_REDUCE_MAX_BLOCKS, grid * sizeof(double), hipMemcpyDeviceToHost, stream));
    Finish();
    double re = 0, im = 0;
    for (int i = 0; i < grid; ++i) {
        re += hPartials[i];
        im += hPartials[QA_REDUCE_MAX_BLOCKS + i];
    }
    if (tmp) freeDev(tmp, maxQPower);
    const double inner = std::sqrt(re * re + im * im);
    return std::max(0.0, 2.0 - 2.0 * inner);
}

// ---- structural -------------------------------------------------------------

template <typename R> bitLenInt QEngineHIP<R>::Compose(QInterfacePtr<R> toCopy, bitLenInt start)
{
    const bitLenInt oQubits = toCopy->GetQubitCount();
    const bitCapInt nMaxQPower = maxQPower << oQubits;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QEngineHIP<R>* o = dynamic_cast<QEngineHIP<R>*>(toCopy.get());
    const cplx<R>* otherBuf = nullptr;
    cplx<R>* tmp = nullptr;
    if (o && o->deviceId == deviceId) {
        otherBuf = o->rState();
        o->Finish();
    } else {
        std::vector<cplx<R>> host(toCopy->GetMaxQPower());
        toCopy->GetQuantumState(host.data());
        tmp = allocDev(toCopy->GetMaxQPower());
        QA_HIP_CHECK(hipMemcpyAsync(tmp, host.data(), sizeof(cplx<R>) * toCopy->GetMaxQPower(),
            hipMemcpyHostToDevice, stream));
        otherBuf = tmp;
    }
    cplx<R>* nBuf = allocDev(nMaxQPower);
    launchCompose<R>(rState(), otherBuf, nBuf, nMaxQPower, start, oQubits, stream);
    Finish();
    if (tmp) freeDev(tmp, toCopy->GetMaxQPower());
    resizeState(nMaxQPower, nBuf);
    this->SetQubitCount(qubitCount + oQubits);
    runningNorm = (R)-1;
    return start;
}

template <typename R> std::vector<double> QEngineHIP<R>::partProbs(bitLenInt start, bitLenInt length)
{
    const bitCapInt partPower = pow2(length);
    QA_HIP_CHECK(hipSetDevice(deviceId));
    double* dProbs = nullptr;
    QA_HIP_CHECK(hipMallocAsync(&dProbs, partPower * sizeof(double), stream));
    QA_HIP_CHECK(hipMemsetAsync(dProbs, 0, partPower * sizeof(double), stream));
    launchPartProbs<R>(rState(), maxQPower, start, length, dProbs, stream);
    std::vector<double> probs(partPower);
    QA_HIP_CHECK(hipMemcpyAsync(
        probs.data(), dProbs, partPower * sizeof(double), hipMemcpyDeviceToHost, stream));
    Finish();
    QA_HIP_CHECK(hipFreeAsync(dProbs, stream));
    return probs;
}

template <typename R> void QEngineHIP<R>::Decompose(bitLenInt start, QInterfacePtr<R> dest)
{
    // Schmidt-rank-1 split on-device (parity: decomposeprob/decomposeamp).
    const bitLenInt len = dest->GetQubitCount();
    const bitLenInt remLen = qubitCount - len;
    const bitCapInt partPower = pow2(len);
    const bitCapInt remPower = pow2(remLen);

    const std::vector<double> pProbs = partProbs(start, len);
    bitCapInt pStar = 0;
    for (bitCapInt p = 1; p < partPower; ++p) {
        if (pProbs[p] > pProbs[pStar]) pStar = p;
    }
    // global max amplitude gives the remainder row with max |a_r|
    const auto mx = argMax();
    const bitCapInt fullIdx = mx.second;
    const bitCapInt lowMask = pow2Mask(start);
    const bitCapInt rStar = (fullIdx & lowMask) | ((fullIdx >> (start + len)) << start);
    // remProb[rStar] via masked reduction (remainder bits = all but the part register)
    const bitCapInt partMask = pow2Mask(len) << start;
    ReduceArgs ra{};
    ra.maxI = maxQPower;
    ra.mask = ~partMask & (maxQPower - 1u);
    ra.perm = (fullIdx & lowMask) | (fullIdx & ~(lowMask | partMask));
    const double remProbStar = reduceSum((int)ReduceOp::PROB_MASK, ra);
    const cplx<R> ampRP = GetAmplitude(fullIdx & ~partMask | (pStar << start));

    const double pNorm = 1.0 / std::sqrt(std::max(1e-300, pProbs[pStar]));
    const double rNorm = 1.0 / std::sqrt(std::max(1e-300, remProbStar));

    // dest amplitudes
    QEngineHIP<R>* od = dynamic_cast<QEngineHIP<R>*>(dest.get());
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* dDest = nullptr;
    bool destLocal = od && od->deviceId == deviceId;
    if (destLocal) {
        dDest = od->wState();
        od->Finish();
    } else {
        QA_HIP_CHECK(hipMallocAsync(&dDest, partPower * sizeof(cplx<R>), stream));
    }
    launchGatherPart<R>(rState(), dDest, partPower, start, len, rStar, cplx<R>((R)rNorm, 0), stream);

    // remainder amplitudes, with the double-counted-phase correction folded in
    cplx<R>* nBuf = allocDev(remPower);
    // corr = orig(rStar,pStar) / (remAmp[rStar] * partAmp[pStar]);
    // remAmp[r] = pNorm * amp(r, pStar), partAmp[p] = rNorm * amp(rStar, p)
    cplx<R> prod = cplx<R>((R)(pNorm * rNorm), 0) * ampRP * ampRP;
    cplx<R> corrScale;
    if (norm(prod) > 0) {
        const std::complex<double> corr =
            std::complex<double>(ampRP.re, ampRP.im) /
            std::complex<double>(prod.re, prod.im);
        corrScale = cplx<R>((R)(corr.real() * pNorm), (R)(corr.imag() * pNorm));
    } else {
        corrScale = cplx<R>((R)pNorm, 0);
    }
    launchDisposeSlice<R>(rState(), nBuf, remPower, start, len, pStar, corrScale, stream);
    Finish();

    if (destLocal) {
        od->runningNorm = (R)-1;
    } else {
        std::vector<cplx<R>> host(partPower);
        QA_HIP_CHECK(hipMemcpyAsync(
            host.data(), dDest, partPower * sizeof(cplx<R>), hipMemcpyDeviceToHost, stream));
        Finish();
        QA_HIP_CHECK(hipFreeAsync(dDest, stream));
        dest->SetQuantumState(host.data());
    }
    resizeState(remPower, nBuf);
    this->SetQubitCount(remLen);
    runningNorm = (R)-1;
    if (doNormalize) NormalizeState();
}

template <typename R> void QEngineHIP<R>::Dispose(bitLenInt start, bitLenInt length)
{
    const std::vector<double> pProbs = partProbs(start, length);
    bitCapInt pStar = 0;
    for (bitCapInt p = 1; p < (bitCapInt)pProbs.size(); ++p) {
        if (pProbs[p] > pProbs[pStar]) pStar = p;
    }
    const double scale = 1.0 / std::sqrt(std::max(1e-300, pProbs[pStar]));
    const bitCapInt remPower = maxQPower >> length;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* nBuf = allocDev(remPower);
    launchDisposeSlice<R>(rState(), nBuf, remPower, start, length, pStar, cplx<R>((R)scale, 0), stream);
    Finish();
    resizeState(remPower, nBuf);
    this->SetQubitCount(qubitCount - length);
    runningNorm = (R)-1;
}

template <typename R>
void QEngineHIP<R>::Dispose(bitLenInt start, bitLenInt length, bitCapInt disposedPerm)
{
    const bitCapInt remPower = maxQPower >> length;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* nBuf = allocDev(remPower);
    launchDisposeSlice<R>(rState(), nBuf, remPower, start, length, disposedPerm, cplx<R>(1, 0), stream);
    Finish();
    resizeState(remPower, nBuf);
    this->SetQubitCount(qubitCount - length);
    runningNorm = (R)-1;
    if (doNormalize) NormalizeState();
}

template <typename R> bitLenInt QEngineHIP<R>::Allocate(bitLenInt start, bitLenInt length)
{
    if (!length) return start;
    const bitCapInt nMaxQPower = maxQPower << length;
    QA_HIP_CHECK(hipSetDevice(deviceId));
    cplx<R>* nBuf = allocDev(nMaxQPower);
    launchAllocateExpand<R>(rState(), nBuf, nMaxQPower, start, length, stream);
    Finish();
    resizeState(nMaxQPower, nBuf);
    this->SetQubitCount(qubitCount + length);
    return start;
}

template <typename R> QInterfacePtr<R> QEngineHIP<R>::Clone()
{
    auto clone = std::make_shared<QEngineHIP<R>>(
        qubitCount, 0u, this->rand_generator, doNormalize, amplitudeFloor, deviceId);
    const cplx<R>* srcBuf = rState();
    Finish();
    QA_HIP_CHECK(hipSetDevice(deviceId));
    QA_HIP_CHECK(hipMemcpyAsync(clone->wStateAll(), srcBuf, sizeof(cplx<R>) * maxQPower,
        hipMemcpyDeviceToDevice, clone->stream));
    clone->Finish();
    clone->runningNorm = runningNorm;
    return clone;
}

// ---- ALU --------------------------------------------------------------------

template <typename R> void QEngineHIP<R>::permuteOp(PermArgs& a, bool partialSpace, bool copyFirst)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    HipProfScope prof("alu_permute", stream);
    ensureScratch();
    if (copyFirst && partialSpace) {
        // controlled op over a sub-domain of the controlled subspace (carry/out
        // register |0>): sources that are nobody's destination must not survive
        launchCopyUncontrolled<R>(rState(), dScratch, maxQPower, a.controlMask, stream);
    } else if (copyFirst) {
        QA_HIP_CHECK(hipMemcpyAsync(
            dScratch, rState(), sizeof(cplx<R>) * maxQPower, hipMemcpyDeviceToDevice, stream));
    } else if (partialSpace) {
        QA_HIP_CHECK(hipMemsetAsync(dScratch, 0, sizeof(cplx<R>) * maxQPower, stream));
    }
    launchPermute<R>(rState(), dScratch, a, stream);
    Finish();
    swapScratch();
}

static void fillSkips(PermArgs& a, std::vector<bitCapInt> powers)
{
    std::sort(powers.begin(), powers.end());
    if ((int)powers.size() > QA_MAX_SKIP_POWERS) throw QrackError("too many fixed qubits in ALU op");
    a.nPowers = (int)powers.size();
    for (int i = 0; i < a.nPowers; ++i) a.qPowers[i] = powers[i];
}

template <typename R>
static void checkAluRangeHip(bitLenInt start, bitLenInt length, bitLenInt qubitCount, const char* op)
{
    if ((bitCapInt)start + length > qubitCount) {
        throw QrackError(std::string(op) + ": register is out of the qubit range");
    }
}

template <typename R> void QEngineHIP<R>::INC(bitCapInt toAdd, bitLenInt start, bitLenInt length)
{
    checkAluRangeHip<R>(start, length, qubitCount, "INC");
    if (!length) return;
    toAdd &= pow2Mask(length);
    if (!toAdd) return;
    PermArgs a{};
    a.op = (int)PermOp::INC;
    a.maxI = maxQPower;
    a.start = start;
    a.length = length;
    a.operand = toAdd;
    permuteOp(a, false, false);
}

template <typename R>
void QEngineHIP<R>::CINC(
    bitCapInt toAdd, bitLenInt start, bitLenInt length, const std::vector<bitLenInt>& controls)
{
    if (controls.empty()) {
        INC(toAdd, start, length);
        return;
    }
    if (!length) return;
    toAdd &= pow2Mask(length);
    if (!toAdd) return;
    PermArgs a{};
    a.op = (int)PermOp::INC;
    a.start = start;
    a.length = length;
    a.operand = toAdd;
    std::vector<bitCapInt> powers;
    for (bitLenInt c : controls) {
        powers.push_back(pow2(c));
        a.controlMask |= pow2(c);
    }
    fillSkips(a, powers);
    a.maxI = maxQPower >> (bitLenInt)controls.size();
    permuteOp(a, false, true);
}

template <typename R>
void QEngineHIP<R>::INCC(bitCapInt toAdd, bitLenInt start, bitLenInt length, bitLenInt carryIndex)
{
    const bool hasCarry = this->M(carryIndex);
    if (hasCarry) {
        this->X(carryIndex);
        ++toAdd;
    }
    if (!length) return;
    PermArgs a{};
    a.op = (int)PermOp::INCDECC;
    a.start = start;
    a.length = length;
    a.operand = toAdd & pow2Mask(length);
    a.carryMask = pow2(carryIndex);
    fillSkips(a, { a.carryMask });
    a.maxI = maxQPower >> 1u;
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::DECC(bitCapInt toSub, bitLenInt start, bitLenInt length, bitLenInt carryIndex)
{
    const bool hasCarry = this->M(carryIndex);
    bitCapInt invToSub = (pow2(length) - toSub) & pow2Mask(length);
    if (hasCarry) {
        this->X(carryIndex);
    } else {
        invToSub = (invToSub - 1u) & pow2Mask(length);
    }
    if (!length) return;
    PermArgs a{};
    a.op = (int)PermOp::INCDECC;
    a.start = start;
    a.length = length;
    a.operand = invToSub;
    a.carryMask = pow2(carryIndex);
    fillSkips(a, { a.carryMask });
    a.maxI = maxQPower >> 1u;
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::INCS(bitCapInt toAdd, bitLenInt start, bitLenInt length, bitLenInt overflowIndex)
{
    if (!length) return;
    toAdd &= pow2Mask(length);
    if (!toAdd) return;
    PermArgs a{};
    a.op = (int)PermOp::INCS;
    a.maxI = maxQPower;
    a.start = start;
    a.length = length;
    a.operand = toAdd;
    a.carryMask = pow2(overflowIndex);
    permuteOp(a, false, false);
}

template <typename R>
void QEngineHIP<R>::INCBCD(bitCapInt toAdd, bitLenInt start, bitLenInt length)
{
    if (length % 4u) throw QrackError("INCBCD: length must be a multiple of 4");
    checkAluRangeHip<R>(start, length, qubitCount, "INCBCD");
    const bitLenInt digits = length / 4u;
    bitCapInt tenPow = 1;
    for (bitLenInt i = 0; i < digits; ++i) tenPow *= 10u;
    toAdd %= tenPow;
    if (!toAdd) return;
    PermArgs a{};
    a.op = (int)PermOp::INCBCD;
    a.maxI = maxQPower;
    a.start = start;
    a.length = length;
    a.operand = toAdd;
    permuteOp(a, false, false);
}

template <typename R>
void QEngineHIP<R>::MUL(bitCapInt toMul, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length)
{
    if (!toMul) throw QrackError("MUL by zero is not invertible");
    if (toMul == 1u) return;
    PermArgs a{};
    a.op = (int)PermOp::MUL;
    a.start = inOutStart;
    a.length = length;
    a.start2 = carryStart;
    a.operand = toMul;
    std::vector<bitCapInt> powers;
    for (bitLenInt i = 0; i < length; ++i) powers.push_back(pow2(carryStart + i));
    fillSkips(a, powers);
    a.maxI = maxQPower >> length;
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::DIV(bitCapInt toDiv, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length)
{
    if (!toDiv) throw QrackError("DIV by zero");
    if (toDiv == 1u) return;
    PermArgs a{};
    a.op = (int)PermOp::DIV;
    a.start = inOutStart;
    a.length = length;
    a.start2 = carryStart;
    a.operand = toDiv;
    std::vector<bitCapInt> powers;
    for (bitLenInt i = 0; i < length; ++i) powers.push_back(pow2(carryStart + i));
    fillSkips(a, powers);
    a.maxI = maxQPower >> length;
    permuteOp(a, true, false);
}

template <typename R>
static void setupModArgs(PermArgs& a, PermOp op, bitCapInt operand, bitCapInt modN, bitLenInt inStart,
    bitLenInt outStart, bitLenInt length, bitCapInt maxQPower, const std::vector<bitLenInt>& controls)
{
    a.op = (int)op;
    a.start = inStart;
    a.length = length;
    a.start2 = outStart;
    a.length2 = length;
    a.operand = operand;
    a.modN = modN;
    std::vector<bitCapInt> powers;
    for (bitLenInt i = 0; i < length; ++i) powers.push_back(pow2(outStart + i));
    for (bitLenInt c : controls) {
        powers.push_back(pow2(c));
        a.controlMask |= pow2(c);
    }
    fillSkips(a, powers);
    a.maxI = maxQPower >> (length + (bitLenInt)controls.size());
}

template <typename R>
void QEngineHIP<R>::MULModNOut(
    bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart, bitLenInt length)
{
    qaCheckModN<R>(modN, length, "MULModNOut");
    checkAluRangeHip<R>(inStart, length, qubitCount, "MULModNOut");
    checkAluRangeHip<R>(outStart, length, qubitCount, "MULModNOut");
    PermArgs a{};
    setupModArgs<R>(a, PermOp::MULMODN, toMul, modN, inStart, outStart, length, maxQPower, {});
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::IMULModNOut(
    bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart, bitLenInt length)
{
    qaCheckModN<R>(modN, length, "IMULModNOut");
    PermArgs a{};
    setupModArgs<R>(a, PermOp::IMULMODN, toMul, modN, inStart, outStart, length, maxQPower, {});
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::POWModNOut(
    bitCapInt base, bitCapInt modN, bitLenInt inStart, bitLenInt outStart, bitLenInt length)
{
    qaCheckModN<R>(modN, length, "POWModNOut");
    checkAluRangeHip<R>(inStart, length, qubitCount, "POWModNOut");
    checkAluRangeHip<R>(outStart, length, qubitCount, "POWModNOut");
    PermArgs a{};
    setupModArgs<R>(a, PermOp::POWMODN, base, modN, inStart, outStart, length, maxQPower, {});
    permuteOp(a, true, false);
}

template <typename R>
void QEngineHIP<R>::CMUL(bitCapInt toMul, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length,
    const std::vector<bitLenInt>& controls)
{
    if (controls.empty()) {
        MUL(toMul, inOutStart, carryStart, length);
        return;
    }
    if (!toMul) throw QrackError("CMUL by zero is not invertible");
    if (toMul == 1u) return;
    PermArgs a{};
    a.op = (int)PermOp::MUL;
    a.start = inOutStart;
    a.length = length;
    a.start2 = carryStart;
    a.operand = toMul;
    std::vector<bitCapInt> powers;
    for (bitLenInt i = 0; i < length; ++i) powers.push_back(pow2(carryStart + i));
    for (bitLenInt c : controls) {
        powers.push_back(pow2(c));
        a.controlMask |= pow2(c);
    }
    fillSkips(a, powers);
    a.maxI = maxQPower >> (length + (bitLenInt)controls.size());
    permuteOp(a, true, true);
}

template <typename R>
void QEngineHIP<R>::CDIV(bitCapInt toDiv, bitLenInt inOutStart, bitLenInt carryStart, bitLenInt length,
    const std::vector<bitLenInt>& controls)
{
    if (controls.empty()) {
        DIV(toDiv, inOutStart, carryStart, length);
        return;
    }
    if (!toDiv) throw QrackError("CDIV by zero");
    if (toDiv == 1u) return;
    PermArgs a{};
    a.op = (int)PermOp::DIV;
    a.start = inOutStart;
    a.length = length;
    a.start2 = carryStart;
    a.operand = toDiv;
    std::vector<bitCapInt> powers;
    for (bitLenInt i = 0; i < length; ++i) powers.push_back(pow2(carryStart + i));
    for (bitLenInt c : controls) {
        powers.push_back(pow2(c));
        a.controlMask |= pow2(c);
    }
    fillSkips(a, powers);
    a.maxI = maxQPower >> (length + (bitLenInt)controls.size());
    permuteOp(a, true, true);
}

template <typename R>
void QEngineHIP<R>::CMULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
    bitLenInt length, const std::vector<bitLenInt>& controls)
{
    qaCheckModN<R>(modN, length, "CMULModNOut");
    if (controls.empty()) {
        MULModNOut(toMul, modN, inStart, outStart, length);
        return;
    }
    PermArgs a{};
    setupModArgs<R>(a, PermOp::MULMODN, toMul, modN, inStart, outStart, length, maxQPower, controls);
    permuteOp(a, true, true);
}

template <typename R>
void QEngineHIP<R>::CIMULModNOut(bitCapInt toMul, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
    bitLenInt length, const std::vector<bitLenInt>& controls)
{
    qaCheckModN<R>(modN, length, "CIMULModNOut");
    if (controls.empty()) {
        IMULModNOut(toMul, modN, inStart, outStart, length);
        return;
    }
    PermArgs a{};
    setupModArgs<R>(a, PermOp::IMULMODN, toMul, modN, inStart, outStart, length, maxQPower, controls);
    permuteOp(a, true, true);
}

template <typename R>
void QEngineHIP<R>::CPOWModNOut(bitCapInt base, bitCapInt modN, bitLenInt inStart, bitLenInt outStart,
    bitLenInt length, const std::vector<bitLenInt>& controls)
{
    qaCheckModN<R>(modN, length, "CPOWModNOut");
    if (controls.empty()) {
        POWModNOut(base, modN, inStart, outStart, length);
        return;
    }
    PermArgs a{};
    setupModArgs<R>(a, PermOp::POWMODN, base, modN, inStart, outStart, length, maxQPower, controls);
    permuteOp(a, true, true);
}

template <typename R> unsigned char* QEngineHIP<R>::uploadTable(const unsigned char* values, size_t bytes)
{
    QA_HIP_CHECK(hipStreamSynchronize(stream)); // hAux_ and dAux_ are free again
    hAux_.assign(values, values + bytes);
    return uploadAux(bytes);
}

template <typename R>
bitCapInt QEngineHIP<R>::IndexedLDA(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
    bitLenInt valueLength, const unsigned char* values, bool resetValue)
{
    if (resetValue) {
        const int bytes = (int)((valueLength + 7u) / 8u);
        unsigned char* dTable =
            uploadTable(values, ((size_t)1 << indexLength) * bytes);
        PermArgs a{};
        a.op = (int)PermOp::LDA;
        a.start = indexStart;
        a.length = indexLength;
        a.start2 = valueStart;
        a.length2 = valueLength;
        a.table = dTable;
        a.tableBytes = bytes;
        std::vector<bitCapInt> powers;
        for (bitLenInt i = 0; i < valueLength; ++i) powers.push_back(pow2(valueStart + i));
        fillSkips(a, powers);
        a.maxI = maxQPower >> valueLength;
        permuteOp(a, true, false);
    }
    std::vector<bitLenInt> bits;
    for (bitLenInt i = 0; i < valueLength; ++i) bits.push_back(valueStart + i);
    return (bitCapInt)(this->ExpectationBitsAll(bits) + 0.5);
}

template <typename R>
bitCapInt QEngineHIP<R>::IndexedADC(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
    bitLenInt valueLength, bitLenInt carryIndex, const unsigned char* values)
{
    const bool hasCarry = this->M(carryIndex);
    bitCapInt extra = 0;
    if (hasCarry) {
        this->X(carryIndex);
        extra = 1;
    }
    const int bytes = (int)((valueLength + 7u) / 8u);
    unsigned char* dTable =
        uploadTable(values, ((size_t)1 << indexLength) * bytes);
    PermArgs a{};
    a.op = (int)PermOp::ADC;
    a.start = indexStart;
    a.length = indexLength;
    a.start2 = valueStart;
    a.length2 = valueLength;
    a.carryMask = pow2(carryIndex);
    a.extra = extra;
    a.table = dTable;
    a.tableBytes = bytes;
    fillSkips(a, { a.carryMask });
    a.maxI = maxQPower >> 1u;
    permuteOp(a, true, false);
    std::vector<bitLenInt> bits;
    for (bitLenInt i = 0; i < valueLength; ++i) bits.push_back(valueStart + i);
    return (bitCapInt)(this->ExpectationBitsAll(bits) + 0.5);
}

template <typename R>
bitCapInt QEngineHIP<R>::IndexedSBC(bitLenInt indexStart, bitLenInt indexLength, bitLenInt valueStart,
    bitLenInt valueLength, bitLenInt carryIndex, const unsigned char* values)
{
    const bool hasCarry = this->M(carryIndex);
    bitCapInt extra = 0;
    if (hasCarry) {
        this->X(carryIndex);
    } else {
        extra = (bitCapInt)0 - 1u;
    }
    const int bytes = (int)((valueLength + 7u) / 8u);
    unsigned char* dTable =
        uploadTable(values, ((size_t)1 << indexLength) * bytes);
    PermArgs a{};
    a.op = (int)PermOp::SBC;
    a.start = indexStart;
    a.length = indexLength;
    a.start2 = valueStart;
    a.length2 = valueLength;
    a.carryMask = pow2(carryIndex);
    a.extra = extra;
    a.table = dTable;
    a.tableBytes = bytes;
    fillSkips(a, { a.carryMask });
    a.maxI = maxQPower >> 1u;
    permuteOp(a, true, false);
    std::vector<bitLenInt> bits;
    for (bitLenInt i = 0; i < valueLength; ++i) bits.push_back(valueStart + i);
    return (bitCapInt)(this->ExpectationBitsAll(bits) + 0.5);
}

template <typename R>
void QEngineHIP<R>::Hash(bitLenInt start, bitLenInt length, const unsigned char* values)
{
    const int bytes = (int)((length + 7u) / 8u);
    unsigned char* dTable = uploadTable(values, ((size_t)1 << length) * bytes);
    PermArgs a{};
    a.op = (int)PermOp::HASH;
    a.maxI = maxQPower;
    a.start = start;
    a.length = length;
    a.table = dTable;
    a.tableBytes = bytes;
    permuteOp(a, false, false);
}

template <typename R> void QEngineHIP<R>::ROL(bitLenInt shift, bitLenInt start, bitLenInt length)
{
    if (!length) return;
    shift %= length;
    if (!shift) return;
    PermArgs a{};
    a.op = (int)PermOp::ROL;
    a.maxI = maxQPower;
    a.start = start;
    a.length = length;
    a.operand = shift;
    permuteOp(a, false, false);
}

template <typename R>
void QEngineHIP<R>::PhaseFlipIfLess(bitCapInt greaterPerm, bitLenInt start, bitLenInt length)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchPhaseFlipIfLess<R>(
        wState(), maxQPower, greaterPerm, start, pow2Mask(length) << start, 0u, stream);
}

template <typename R>
void QEngineHIP<R>::CPhaseFlipIfLess(
    bitCapInt greaterPerm, bitLenInt start, bitLenInt length, bitLenInt flagIndex)
{
    QA_HIP_CHECK(hipSetDevice(deviceId));
    launchPhaseFlipIfLess<R>(
        wState(), maxQPower, greaterPerm, start, pow2Mask(length) << start, pow2(flagIndex), stream);
}

size_t HipActiveAllocImpl(int device)
{
    auto& t = HipDeviceTracker::instance();
    if (device < 0 || device >= t.deviceCount()) return 0;
    return t.activeAlloc(device);
}

// ---- factory hook -----------------------------------------------------------

template <typename R>
QInterfacePtr<R> MakeHipEngine(bitLenInt qubits, bitCapInt initPerm, RngPtr rng, int64_t deviceId)
{
    return std::make_shared<QEngineHIP<R>>(
        qubits, initPerm, rng, true, eps<R>::value, deviceId);
}

template QInterfacePtr<float> MakeHipEngine<float>(bitLenInt, bitCapInt, RngPtr, int64_t);
template QInterfacePtr<double> MakeHipEngine<double>(bitLenInt, bitCapInt, RngPtr, int64_t);

template class QEngineHIP<float>;
template class QEngineHIP<double>;

} // namespace qrack_amd
