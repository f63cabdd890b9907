// Sanitizer lane (the reference has no ASAN/TSAN hooks; this
// build adds one): a C++-level battery over the layer stacks, built with
// -fsanitize=address,undefined by `make asan` and run on CPU.
#include "../csrc/qbdt.hpp"
#include "../csrc/qengine_cpu.hpp"
#include "../csrc/qengine_sparse.hpp"
#include "../csrc/qfactory.hpp"
#include "../csrc/qpager.hpp"
#include "../csrc/qstabilizerhybrid.hpp"
#include "../csrc/qunit.hpp"

#include <cstdio>

using namespace qrack_amd;

static void battery(QInterfacePtr<float> q)
{
    const bitLenInt n = q->GetQubitCount();
    q->H(0);
    for (bitLenInt i = 0; i + 1 < n; ++i) q->CNOT(i, i + 1);
    q->T(1);
    q->RY(0.3f, 2);
    q->Swap(0, n - 1);
    q->QFT(0, n);
    q->IQFT(0, n);
    (void)q->Prob(n - 1);
    auto res = q->MultiShotMeasureMask({ 1u, 2u, 4u }, 50);
    (void)q->MAll();
    q->SetPermutation(3);
    try {
        q->INC(2, 0, n - 1);
    } catch (const QrackError&) {
        // some stacks (pure BDT) have no ALU: expected capability hole
    }
    // batched 1q gates + SDRP approximate mode
    const float s2 = 0.70710678f;
    const cplx<float> hh[4] = { { s2, 0 }, { s2, 0 }, { s2, 0 }, { -s2, 0 } };
    std::vector<cplx<float>> ms;
    for (int g = 0; g < 3; ++g) ms.insert(ms.end(), hh, hh + 4);
    q->Mtrx1qBatch({ 0, 2, 4 }, ms);
    q->SetSdrp(0.3);
    q->H(1);
    q->CNOT(1, 3);
    q->RY(0.05f, 3);
    q->CZ(1, 3);
    (void)q->GetUnitaryFidelity();
    q->SetSdrp(0.0);
    // round-2 paths: T-gadget ancillae + buffered cross-unit CX + wide masks
    q->SetPermutation(0);
    q->H(0);
    q->T(0);
    q->CNOT(0, 1);
    q->H(2);
    q->CNOT(2, 3);
    q->CNOT(2, 3);
    (void)q->Prob(1);
    BigCap wide = q->MAllWide();
    (void)wide;
    q->SetPermutationWide(BigCap(5, 0));
    (void)q->MultiShotMeasureQubits({ 0, 3, 5 }, 8);
    (void)res;
}

int main()
{
    const std::vector<std::vector<std::string>> stacks = {
        { "cpu" },
        { "sparse" },
        { "bdt" },
        { "stabilizer_hybrid", "cpu" },
        { "qunit", "cpu" },
        { "qunit", "stabilizer_hybrid", "cpu" },
        { "pager", "cpu" },
        { "turboquant" },
        { "qunit", "stabilizer_hybrid", "turboquant" },
    };
    for (const auto& layers : stacks) {
        auto q = CreateStack<float>(6, layers, 0, 42, -1, 2);
        battery(q);
        std::printf("ok:");
        for (auto& l : layers) std::printf(" %s", l.c_str());
        std::printf("\n");
    }
    // exercise clone/compose/decompose lifecycles under the sanitizer
    auto a = CreateStack<float>(3, { "cpu" }, 0, 1, -1, 1);
    auto b = CreateStack<float>(2, { "cpu" }, 0, 2, -1, 1);
    a->H(0);
    b->X(0);
    a->Compose(b);
    auto c = a->Clone();
    auto dest = CreateStack<float>(2, { "cpu" }, 0, 3, -1, 1);
    c->Decompose(3, dest);
    std::printf("ok: lifecycle\n");
    // QEngineCPU one-pass Pauli strings and sums: widths 1, 2, 5 and 13 (the
    // last one is wide enough for the thread pool), every x-mask shape
    for (bitLenInt n : { 1u, 2u, 5u, 13u }) {
        auto p = CreateStack<float>(n, { "cpu" }, 0, 4, -1, 1);
        for (bitLenInt i = 0; i < n; ++i) p->RY(0.3f + 0.1f * (float)i, i);
        for (bitLenInt i = 0; i + 1 < n; ++i) p->CNOT(i, i + 1);
        std::vector<PauliTerm> terms;
        terms.push_back({ 0.5, {}, {} });
        terms.push_back({ 1.0, { 0 }, { PauliX } });
        terms.push_back({ -1.0, { n - 1 }, { PauliY } });
        if (n > 1) {
            terms.push_back({ 0.25, { n - 1, 0 }, { PauliZ, PauliI } });
            terms.push_back({ 0.75, { 0, n - 1 }, { PauliY, PauliY } });
            terms.push_back({ 0.75, { n - 1, 0 }, { PauliX, PauliX } });
            terms.push_back({ 2.0, { 0, 1 }, { PauliZ, PauliZ } });
        }
        std::vector<bitLenInt> all;
        std::vector<Pauli> mixed;
        for (bitLenInt i = 0; i < n; ++i) {
            all.push_back(i);
            mixed.push_back((Pauli)(1 + i % 3));
        }
        terms.push_back({ 1.5, all, mixed });
        terms.push_back({ 1.5, all, mixed }); // merges with the one before
        const double e = p->ExpectationPauliSum(terms);
        double ref = 0;
        for (const PauliTerm& t : terms) ref += t.coeff * p->PauliExpectation(t.bits, t.paulis);
        if (std::abs(e - ref) > 1e-5) {
            std::printf("FAIL: pauli sum %u: %f vs %f\n", n, e, ref);
            return 1;
        }
        (void)p->ExpectationPauliAll(all, mixed);
        (void)p->VariancePauliAll(all, mixed);
        (void)p->PauliExpectation({ 0, 0 }, { PauliX, PauliZ }); // repeated qubit: generic path
        try {
            (void)p->ExpectationPauliSum({ { 1.0, { n }, { PauliX } } });
            std::printf("FAIL: out-of-range qubit accepted\n");
            return 1;
        } catch (const QrackError&) {
        }
        // the one-pass evolution against the generic lowering of the same
        // product (QUnit over the CPU engine), second order so that passes merge
        auto g = CreateStack<float>(n, { "qunit", "cpu" }, 0, 4, -1, 1);
        for (bitLenInt i = 0; i < n; ++i) g->RY(0.3f + 0.1f * (float)i, i);
        for (bitLenInt i = 0; i + 1 < n; ++i) g->CNOT(i, i + 1);
        p->EvolvePauliSum(terms, 0.1, 3, 2);
        g->EvolvePauliSum(terms, 0.1, 3, 2);
        p->PauliRotation(all, mixed, 0.2);
        g->PauliRotation(all, mixed, 0.2);
        std::vector<cplx<float>> sp(pow2(n)), sg(pow2(n));
        p->GetQuantumState(sp.data());
        g->GetQuantumState(sg.data());
        for (size_t k = 0; k < sp.size(); ++k) {
            if (std::abs(sp[k].re - sg[k].re) > 1e-4f || std::abs(sp[k].im - sg[k].im) > 1e-4f) {
                std::printf("FAIL: pauli evolve %u at %zu\n", n, k);
                return 1;
            }
        }
        try {
            p->EvolvePauliSum(terms, 0.1, 0, 1);
            std::printf("FAIL: steps = 0 accepted\n");
            return 1;
        } catch (const QrackError&) {
        }
    }
    std::printf("ok: pauli sum and evolution\n");
    return 0;
}
