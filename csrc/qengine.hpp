// qrack_amd — abstract Schrödinger state-vector engine.
//
// Capability parity target: /root/reference/include/qengine.hpp (Apply2x2,
// GetAmplitudePage/SetAmplitudePage, ShuffleBuffers, ApplyM contract) plus
// the shared gate→Apply2x2 lowering of /root/reference/src/qengine/qengine.cpp.
// Fresh design: the single primitive is
//   Apply2x2(offset1, offset2, m, qPowersSorted)
// — apply the 2x2 `m` to amplitude pairs (i|offset1, i|offset2) where i
// ranges over indices with all qPowersSorted bits clear. Every controlled /
// swap-family gate lowers onto it; engines specialize diagonal (phase) and
// antidiagonal (invert) matrices internally.
#pragma once

#include "krylov.hpp"
#include "qinterface.hpp"

#include <algorithm>
#include <cmath>

namespace qrack_amd {

// ---- Pauli-sum canonical form (shared by the dense engines) -----------------
//
// A Pauli string is (x, z, ny): x = mask of X/Y factors, z = mask of Z/Y
// factors, ny = number of Y factors. P|i> = i^ny (-1)^popcount(i&z) |i^x>, so
//   <psi|P|psi> = sum_i i^ny (-1)^popcount(i&z) conj(psi[i^x]) psi[i],
// one read-only pass. Terms that share x differ only in a per-index weight
// and share a pass; they are grouped here so engines cannot drift.
struct PauliCanonTerm {
    bitCapInt z;
    double w; // coeff * i^ny, which is purely real or purely imaginary
};

struct PauliGroup {
    bitCapInt x = 0;
    std::vector<PauliCanonTerm> re; // ny even: weight w
    std::vector<PauliCanonTerm> im; // ny odd: weight i*w
};

struct PauliCanonSum {
    double identity = 0;            // summed coefficients of all-identity terms
    std::vector<PauliGroup> groups; // ascending x; an x = 0 group comes first
};

// true when the string can take the one-pass path: every qubit in range and
// none listed twice (callers fall back to the generic lowering otherwise)
inline bool pauliStringMasks(const std::vector<bitLenInt>& bits, const std::vector<Pauli>& paulis,
    bitLenInt qubitCount, bitCapInt& x, bitCapInt& z)
{
    x = 0;
    z = 0;
    bitCapInt seen = 0;
    for (size_t i = 0; i < bits.size(); ++i) {
        if (bits[i] >= qubitCount || bits[i] >= 64u || (unsigned)paulis[i] > 3u) return false;
        const bitCapInt p = pow2(bits[i]);
        if (seen & p) return false;
        seen |= p;
        // PauliX = 1, PauliZ = 2, PauliY = 3: bit 0 flips, bit 1 signs
        if (paulis[i] & 1u) x |= p;
        if (paulis[i] & 2u) z |= p;
    }
    return true;
}

// add coeff * (the string with sign mask z) to a group: weight coeff * i^ny
inline void pauliGroupAdd(PauliGroup& g, bitCapInt z, double coeff)
{
    const int ny = __builtin_popcountll(g.x & z) & 3;
    const double w = (ny & 2) ? -coeff : coeff; // i^2 = -1, i^3 = -i
    ((ny & 1) ? g.im : g.re).push_back({ z, w });
}

inline PauliGroup pauliStringGroup(bitCapInt x, bitCapInt z, double coeff)
{
    PauliGroup g;
    g.x = x;
    pauliGroupAdd(g, z, coeff);
    return g;
}

// Drop identities, merge equal (x, z), group by x. Terms are validated first.
inline PauliCanonSum canonicalizePauliSum(const std::vector<PauliTerm>& terms, bitLenInt qubitCount,
    const char* what = "ExpectationPauliSum")
{
    validatePauliTerms(terms, qubitCount, what);
    std::map<std::pair<bitCapInt, bitCapInt>, double> merged;
    PauliCanonSum out;
    for (const PauliTerm& t : terms) {
        bitCapInt x, z;
        if (!pauliStringMasks(t.bits, t.paulis, qubitCount, x, z))
            throw QrackError(std::string(what) + ": qubit out of range");
        if (!x && !z) {
            out.identity += t.coeff;
        } else {
            merged[{ x, z }] += t.coeff;
        }
    }
    for (const auto& kv : merged) {
        const bitCapInt x = kv.first.first, z = kv.first.second;
        if (out.groups.empty() || out.groups.back().x != x) {
            out.groups.emplace_back();
            out.groups.back().x = x;
        }
        pauliGroupAdd(out.groups.back(), z, kv.second);
    }
    return out;
}

// L and S of the Krylov calls (krylov.hpp): the launches of one pass over a
// canonical sum on the HIP engine, one per (group, chunk of `cap` terms) and
// one for identities alone, and |identity| plus the summed |weight|.
// PAULI_SUM_LAUNCH_TERMS is the HIP launch table's size: the HIP engine
// asserts that it equals QA_PAULI_MAX_TERMS, so that every engine uses one L.
constexpr size_t PAULI_SUM_LAUNCH_TERMS = 32;

inline size_t pauliSumLaunchCount(const PauliCanonSum& c, size_t cap = PAULI_SUM_LAUNCH_TERMS)
{
    size_t n = 0;
    for (const PauliGroup& g : c.groups) n += (g.re.size() + g.im.size() + cap - 1u) / cap;
    return n ? n : 1u;
}

inline double pauliSumAbsWeights(const PauliCanonSum& c)
{
    double s = std::abs(c.identity);
    for (const PauliGroup& g : c.groups) {
        for (const PauliCanonTerm& t : g.re) s += std::abs(t.w);
        for (const PauliCanonTerm& t : g.im) s += std::abs(t.w);
    }
    return s;
}

// ---- Pauli-sum evolution plan (shared by the dense engines) -----------------
//
// EvolvePauliSum is a product of per-term rotations (qinterface.hpp). All
// terms of one group act inside the pairs {i, i^x}, and each parity set of a
// group commutes, so one in-place pass over the state serves a run of
// consecutive factors of one group. A pass is a short list of segments, each
// one parity set rotated by its own tau:
//   re set: (a, b) <- (c a - i s b, c b - i s a),  c + i s = e^{i tau wr(i)}
//   im set: (a, b) <- (c a - s b,   c b + s a),    c + i s = e^{i tau wi(i)}
// with a = psi[i], b = psi[i^x], i in the half-space with the top bit of x
// clear, and wr / wi the signed weight sums of the set at i. The x = 0 group
// is diagonal: psi[i] *= e^{-i tau wr(i)}.
//
// Adjacent passes on one group merge. Segments of the same set add their
// angles; the two sets of a mixed group do not commute, so there the merged
// pass keeps them as alternating segments (re im re at the turn-around of a
// second-order step, im re im across a step boundary) — still one pass.
struct PauliEvolveSeg {
    bool im;    // which parity set of the group
    double tau; // rotation angle per unit weight
};

struct PauliEvolvePass {
    size_t group; // index into PauliCanonSum::groups
    std::vector<PauliEvolveSeg> segs;
};

struct PauliEvolvePlan {
    double phase = 0; // the state is also multiplied by e^{-i phase}
    std::vector<PauliEvolvePass> passes;
};

// segments one pass may hold; a longer alternating run starts a new pass
constexpr size_t PAULI_EVOLVE_MAX_SEGS = 4;

inline PauliEvolvePlan pauliEvolvePlan(const PauliCanonSum& c, double time, int steps, int order)
{
    if (order != 1 && order != 2) throw QrackError("EvolvePauliSum: order must be 1 or 2");
    if (steps < 1) throw QrackError("EvolvePauliSum: steps must be at least 1");
    PauliEvolvePlan plan;
    // the identity term commutes with everything: one scalar for the whole call
    plan.phase = time * c.identity;
    struct Factor {
        size_t group;
        bool im;
    };
    std::vector<Factor> forward;
    for (size_t g = 0; g < c.groups.size(); ++g) {
        if (!c.groups[g].re.empty()) forward.push_back({ g, false });
        if (!c.groups[g].im.empty()) forward.push_back({ g, true });
    }
    const double tau = time / steps;
    auto push = [&plan](const Factor& f, double t) {
        if (!plan.passes.empty() && plan.passes.back().group == f.group) {
            std::vector<PauliEvolveSeg>& segs = plan.passes.back().segs;
            if (segs.back().im == f.im) {
                segs.back().tau += t;
                return;
            }
            if (segs.size() < PAULI_EVOLVE_MAX_SEGS) {
                segs.push_back({ f.im, t });
                return;
            }
        }
        plan.passes.push_back({ f.group, { { f.im, t } } });
    };
    for (int s = 0; s < steps; ++s) {
        if (order == 1) {
            for (const Factor& f : forward) push(f, tau);
        } else {
            for (const Factor& f : forward) push(f, tau / 2);
            for (size_t k = forward.size(); k-- > 0u;) push(forward[k], tau / 2);
        }
    }
    return plan;
}

// Flatten one pass into (z, tau * w) entries, segment by segment, for the
// engines' per-pair loops. segEnd[k] is the end of segment k in the list.
struct PauliEvolveFlat {
    std::vector<bitCapInt> z;
    std::vector<double> w;
    std::vector<size_t> segEnd;
    std::vector<bool> segIm;
};

inline PauliEvolveFlat pauliEvolveFlatten(const PauliCanonSum& c, const PauliEvolvePass& p)
{
    PauliEvolveFlat f;
    const PauliGroup& g = c.groups[p.group];
    for (const PauliEvolveSeg& s : p.segs) {
        for (const PauliCanonTerm& t : (s.im ? g.im : g.re)) {
            f.z.push_back(t.z);
            f.w.push_back(s.tau * t.w);
        }
        f.segEnd.push_back(f.z.size());
        f.segIm.push_back(s.im);
    }
    return f;
}

template <typename R> class QEngine;
template <typename R> using QEnginePtr = std::shared_ptr<QEngine<R>>;

template <typename R> class QEngine : public QInterface<R> {
protected:
    using QInterface<R>::qubitCount;
    using QInterface<R>::maxQPower;
    using QInterface<R>::doNormalize;
    using QInterface<R>::amplitudeFloor;
    R runningNorm;

public:
    QEngine(bitLenInt qBitCount, RngPtr rgp = nullptr, bool doNorm = true,
        R normThresh = eps<R>::value)
        : QInterface<R>(qBitCount, rgp, doNorm, normThresh)
        , runningNorm((R)1)
    {
    }

    R GetRunningNorm()
    {
        this->Finish();
        return runningNorm;
    }

    // ---- THE engine primitive ----------------------------------------------
    virtual void Apply2x2(bitCapInt offset1, bitCapInt offset2, const cplx<R>* mtrx,
        const std::vector<bitCapInt>& qPowersSorted) = 0;

    // measurement collapse: project onto (i & regMask) == result, scaling
    // survivors by nrm (parity: qengine.hpp ApplyM / applym kernel)
    virtual void ApplyM(bitCapInt regMask, bitCapInt result, cplx<R> nrm) = 0;

    // page access for QPager / engine migration
    virtual void GetAmplitudePage(cplx<R>* pagePtr, bitCapInt offset, bitCapInt length) = 0;
    virtual void SetAmplitudePage(const cplx<R>* pagePtr, bitCapInt offset, bitCapInt length) = 0;
    virtual void SetAmplitudePage(
        QEnginePtr<R> pageEnginePtr, bitCapInt srcOffset, bitCapInt dstOffset, bitCapInt length) = 0;
    // swap the halves of two engines' buffers (the QPager cross-page primitive)
    virtual void ShuffleBuffers(QEnginePtr<R> engine) = 0;
    virtual void ZeroAmplitudes() = 0;
    virtual void CopyStateVec(QEnginePtr<R> src) = 0;
    virtual bool IsZeroAmplitude() = 0;

    // ---- gate API lowering --------------------------------------------------
    using QInterface<R>::Mtrx;

    void Mtrx(const cplx<R>* mtrx, bitLenInt target) override
    {
        const bitCapInt targetPower = pow2(target);
        Apply2x2(0u, targetPower, mtrx, { targetPower });
    }

    void UCMtrx(const std::vector<bitLenInt>& controls, const cplx<R>* mtrx, bitLenInt target,
        bitCapInt controlPerm) override
    {
        bitCapInt offset = 0;
        std::vector<bitCapInt> qPowers;
        qPowers.reserve(controls.size() + 1u);
        for (size_t i = 0; i < controls.size(); ++i) {
            const bitCapInt p = pow2(controls[i]);
            qPowers.push_back(p);
            if ((controlPerm >> i) & 1u) offset |= p;
        }
        const bitCapInt targetPower = pow2(target);
        qPowers.push_back(targetPower);
        std::sort(qPowers.begin(), qPowers.end());
        Apply2x2(offset, offset | targetPower, mtrx, qPowers);
    }

    void UniformlyControlledSingleBit(
        const std::vector<bitLenInt>& controls, bitLenInt target, const cplx<R>* mtrxs) override;

    void Swap(bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        const cplx<R> m[4] = { { 0, 0 }, { 1, 0 }, { 1, 0 }, { 0, 0 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
    }

    void ISwap(bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        const cplx<R> m[4] = { { 0, 0 }, { 0, 1 }, { 0, 1 }, { 0, 0 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
    }

    void IISwap(bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        const cplx<R> m[4] = { { 0, 0 }, { 0, -1 }, { 0, -1 }, { 0, 0 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
    }

    void SqrtSwap(bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        const cplx<R> m[4] = { { (R)0.5, (R)0.5 }, { (R)0.5, (R)-0.5 }, { (R)0.5, (R)-0.5 },
            { (R)0.5, (R)0.5 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
    }

    void ISqrtSwap(bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        const cplx<R> m[4] = { { (R)0.5, (R)-0.5 }, { (R)0.5, (R)0.5 }, { (R)0.5, (R)0.5 },
            { (R)0.5, (R)-0.5 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
    }

    void FSim(R theta, R phi, bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) throw QrackError("FSim: identical qubits");
        const R c = std::cos(theta), s = std::sin(theta);
        const cplx<R> m[4] = { { c, 0 }, { 0, -s }, { 0, -s }, { c, 0 } };
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        std::vector<bitCapInt> powers{ std::min(p1, p2), std::max(p1, p2) };
        Apply2x2(p1, p2, m, powers);
        this->MCPhase({ q1 }, cplx<R>(1, 0), polar<R>((R)1, -phi), q2);
    }

    void CSwap(const std::vector<bitLenInt>& controls, bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        ControlledSwapBlock(controls, q1, q2, true, false);
    }
    void AntiCSwap(const std::vector<bitLenInt>& controls, bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        ControlledSwapBlock(controls, q1, q2, true, true);
    }
    void CSqrtSwap(const std::vector<bitLenInt>& controls, bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        ControlledSwapBlock(controls, q1, q2, false, false);
    }
    void AntiCSqrtSwap(const std::vector<bitLenInt>& controls, bitLenInt q1, bitLenInt q2) override
    {
        if (q1 == q2) return;
        ControlledSwapBlock(controls, q1, q2, false, true);
    }

    // additive diagonal phase ramp: amp *= exp(i*scale*((x >> rampStart) mod
    // 2^rampBits)) applied where (condPower == 0) || (x & condPower).
    // One fused pass replaces rampBits (controlled-)phase gates; the default
    // lowering is the gate product (engines override with a single kernel).
    virtual void PhaseRamp(R scale, bitLenInt rampStart, bitLenInt rampBits, bitCapInt condPower)
    {
        for (bitLenInt b = 0; b < rampBits; ++b) {
            const cplx<R> f = polar<R>((R)1, scale * (R)pow2(b));
            if (condPower) {
                this->MCPhase({ log2Ocl(condPower) }, cplx<R>(1, 0), f, rampStart + b);
            } else {
                this->Phase(cplx<R>(1, 0), f, rampStart + b);
            }
        }
    }

    // generalized ramp with relocated bits: frac(i) =
    // ((i >> rampStart) & inPlaceRelMask) + sum_k bit(i, sPows[k]) * sWeights[k];
    // amp *= exp(i*scale*frac) on the condPower-set half (everywhere if 0)
    virtual void PhaseRampGeneral(R scale, bitLenInt rampStart, bitCapInt inPlaceRelMask,
        const std::vector<bitCapInt>& sPows, const std::vector<uint64_t>& sWeights,
        bitCapInt condPower)
    {
        // default lowering: product of per-bit (controlled) phases
        bitCapInt m = inPlaceRelMask;
        while (m) {
            const bitLenInt rel = log2Ocl(m & (~m + 1u));
            const cplx<R> f = polar<R>((R)1, scale * (R)pow2(rel));
            if (condPower) {
                this->MCPhase({ log2Ocl(condPower) }, cplx<R>(1, 0), f, rampStart + rel);
            } else {
                this->Phase(cplx<R>(1, 0), f, rampStart + rel);
            }
            m &= m - 1u;
        }
        for (size_t k = 0; k < sPows.size(); ++k) {
            const cplx<R> f = polar<R>((R)1, scale * (R)sWeights[k]);
            if (condPower) {
                this->MCPhase({ log2Ocl(condPower) }, cplx<R>(1, 0), f, log2Ocl(sPows[k]));
            } else {
                this->Phase(cplx<R>(1, 0), f, log2Ocl(sPows[k]));
            }
        }
    }

    // generalized fused QFT column (distributed pager lazy maps): H on
    // `target` + the relocated-bit ramp e^{i(scale*frac + phase0)} applied on
    // the target=1 side — ONE state pass on engines. pre=true applies the
    // ramp before H (IQFT order). Default lowering: H then general ramp.
    virtual void QftColumnGeneral(bitLenInt target, double scale, bitLenInt rampStart,
        bitCapInt inPlaceRelMask, const std::vector<bitCapInt>& sPows,
        const std::vector<uint64_t>& sWeights, double phase0, bool pre)
    {
        const bitCapInt cond = pow2(target);
        auto ramp = [&]() {
            PhaseRampGeneral((R)scale, rampStart, inPlaceRelMask, sPows, sWeights, cond);
            if (phase0 != 0.0) {
                this->Phase(cplx<R>(1, 0), polar<R>(1, (R)phase0), target);
            }
        };
        if (pre) {
            ramp();
            this->H(target);
        } else {
            this->H(target);
            ramp();
        }
    }

    // ---- measurement --------------------------------------------------------
    bool ForceM(bitLenInt qubit, bool result, bool doForce = true, bool doApply = true) override;

protected:
    void ControlledSwapBlock(
        const std::vector<bitLenInt>& controls, bitLenInt q1, bitLenInt q2, bool full, bool anti)
    {
        bitCapInt offset = 0;
        std::vector<bitCapInt> powers;
        powers.reserve(controls.size() + 2u);
        for (bitLenInt c : controls) {
            const bitCapInt p = pow2(c);
            powers.push_back(p);
            if (!anti) offset |= p;
        }
        const bitCapInt p1 = pow2(q1), p2 = pow2(q2);
        powers.push_back(p1);
        powers.push_back(p2);
        std::sort(powers.begin(), powers.end());
        if (full) {
            const cplx<R> m[4] = { { 0, 0 }, { 1, 0 }, { 1, 0 }, { 0, 0 } };
            Apply2x2(offset | p1, offset | p2, m, powers);
        } else {
            const cplx<R> m[4] = { { (R)0.5, (R)0.5 }, { (R)0.5, (R)-0.5 }, { (R)0.5, (R)-0.5 },
                { (R)0.5, (R)0.5 } };
            Apply2x2(offset | p1, offset | p2, m, powers);
        }
    }
};

template <typename R>
void QEngine<R>::UniformlyControlledSingleBit(
    const std::vector<bitLenInt>& controls, bitLenInt target, const cplx<R>* mtrxs)
{
    // Default lowering: one perm-controlled 2x2 per control permutation.
    // Engines override with the single-pass multiplexer kernel.
    const bitCapInt nPerms = pow2((bitLenInt)controls.size());
    for (bitCapInt p = 0; p < nPerms; ++p) {
        this->UCMtrx(controls, mtrxs + 4u * p, target, p);
    }
}

template <typename R>
bool QEngine<R>::ForceM(bitLenInt qubit, bool result, bool doForce, bool doApply)
{
    const R oneProb = this->Prob(qubit);
    bool outcome;
    if (doForce) {
        outcome = result;
    } else {
        outcome = (this->Rand() < (double)oneProb);
    }
    if (doApply) {
        const R prob = outcome ? oneProb : ((R)1 - oneProb);
        if (prob <= 0) throw QrackError("ForceM: impossible measurement outcome");
        const R nrm = (R)1 / std::sqrt(prob);
        ApplyM(pow2(qubit), outcome ? pow2(qubit) : 0u, cplx<R>(nrm, 0));
    }
    return outcome;
}

} // namespace qrack_amd
