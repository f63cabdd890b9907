// qrack_amd — noise-injection wrapper.
// Capability parity target: /root/reference/include/qinterface_noisy.hpp
// (DepolarizingChannelWeak1Qb after each gate; QRACK_GATE_DEPOLARIZATION env).
#pragma once

#include "qwrapper.hpp"

#include <cstdlib>

namespace qrack_amd {

template <typename R> class QInterfaceNoisy : public QInterfaceWrapper<R> {
protected:
    using QInterfaceWrapper<R>::inner;
    R noiseParam;

    void Noise1(bitLenInt q) { inner->DepolarizingChannelWeak1Qb(q, noiseParam); }
    void Noise2(bitLenInt a, bitLenInt b)
    {
        Noise1(a);
        Noise1(b);
    }

public:
    QInterfaceNoisy(bitLenInt n, QInterfacePtr<R> wrapped, R noise = (R)-1, RngPtr rgp = nullptr)
        : QInterfaceWrapper<R>(n, wrapped, rgp)
        , noiseParam(noise)
    {
        if (noiseParam < 0) {
            noiseParam = (R)0.01;
            if (const char* env = std::getenv("QRACK_GATE_DEPOLARIZATION")) {
                noiseParam = (R)std::atof(env);
            }
        }
    }

    void SetNoiseParameter(double np) override { noiseParam = (R)np; }
    double GetNoiseParameter() override { return (double)noiseParam; }

    // per-gate noise injection must see every gate: undo the wrapper's fused
    // forwarding and lower the batch through Mtrx one gate at a time
    void Mtrx1qBatch(const std::vector<bitLenInt>& targets, const std::vector<cplx<R>>& mtrxs) override
    {
        QInterface<R>::Mtrx1qBatch(targets, mtrxs);
    }

    // likewise the Pauli rotations: the generic lowering, gate by gate
    void PauliRotation(
        const std::vector<bitLenInt>& b, const std::vector<Pauli>& p, double theta) override
    {
        QInterface<R>::PauliRotation(b, p, theta);
    }
    void EvolvePauliSum(
        const std::vector<PauliTerm>& t, double time, int steps = 1, int order = 1) override
    {
        QInterface<R>::EvolvePauliSum(t, time, steps, order);
    }
    // the sweep un-applies every op, which random noise channels do not allow;
    // the two read-style calls (PauliSumBraket, PauliSumApplyInto) are the
    // wrapper's plain forwards
    double AdjointGradient(const std::vector<AdjointOp<R>>&, const std::vector<PauliTerm>&,
        std::vector<double>&) override
    {
        throw QrackError("AdjointGradient: not defined under gate noise");
    }
    // a Krylov step is no sequence of gates a noise channel could follow: the
    // two mutating forms are refused, LanczosTridiagonal and the read-only
    // LanczosGroundState are the wrapper's plain forwards
    double KrylovEvolvePauliSum(const std::vector<PauliTerm>&, double, int = 16, int = 1) override
    {
        throw QrackError("KrylovEvolvePauliSum: not defined under gate noise");
    }
    std::pair<double, double> LanczosGroundState(
        const std::vector<PauliTerm>& t, int dim = 32, bool prepare = false) override
    {
        if (prepare) throw QrackError("LanczosGroundState(prepare): not defined under gate noise");
        return inner->LanczosGroundState(t, dim, false);
    }
    // ... and so is the read-only LanczosLowestStates
    KrylovEigenResult LanczosLowestStates(const std::vector<PauliTerm>& t, int nev = 2, int dim = 16,
        double tol = 0.0, int maxRestarts = 64, int prepare = -1) override
    {
        if (prepare >= 0) throw QrackError("LanczosLowestStates(prepare): not defined under gate noise");
        return inner->LanczosLowestStates(t, nev, dim, tol, maxRestarts, -1);
    }

    void Mtrx(const cplx<R>* m, bitLenInt t) override
    {
        inner->Mtrx(m, t);
        Noise1(t);
    }
    void Phase(cplx<R> tl, cplx<R> br, bitLenInt t) override
    {
        inner->Phase(tl, br, t);
        Noise1(t);
    }
    void Invert(cplx<R> tr, cplx<R> bl, bitLenInt t) override
    {
        inner->Invert(tr, bl, t);
        Noise1(t);
    }
    void MCMtrx(const std::vector<bitLenInt>& c, const cplx<R>* m, bitLenInt t) override
    {
        inner->MCMtrx(c, m, t);
        Noise1(t);
        for (bitLenInt q : c) Noise1(q);
    }
    void MACMtrx(const std::vector<bitLenInt>& c, const cplx<R>* m, bitLenInt t) override
    {
        inner->MACMtrx(c, m, t);
        Noise1(t);
        for (bitLenInt q : c) Noise1(q);
    }
    void MtrxN(const std::vector<bitLenInt>& qubits, const cplx<R>* m,
        const std::vector<bitLenInt>& c = {}, bool anti = false) override
    {
        inner->MtrxN(qubits, m, c, anti);
        for (bitLenInt q : qubits) Noise1(q);
        for (bitLenInt q : c) Noise1(q);
    }
    void Swap(bitLenInt a, bitLenInt b) override
    {
        inner->Swap(a, b);
        Noise2(a, b);
    }
    void ISwap(bitLenInt a, bitLenInt b) override
    {
        inner->ISwap(a, b);
        Noise2(a, b);
    }
    void FSim(R th, R ph, bitLenInt a, bitLenInt b) override
    {
        inner->FSim(th, ph, a, b);
        Noise2(a, b);
    }

    QInterfacePtr<R> Clone() override
    {
        return std::make_shared<QInterfaceNoisy<R>>(
            this->qubitCount, inner->Clone(), noiseParam, this->rand_generator);
    }
};

} // namespace qrack_amd
