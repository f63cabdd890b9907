// Sanitizer lane for the adjoint-gradient calls: a stand-alone program over
// the CPU engine, built with -fsanitize=address,undefined by `make
// asan-adjoint` and run on the CPU. A 6-qubit gradient (rotations, gates, an
// untrainable rotation) checked against central differences of the energy, a
// braket and an H|psi>, in both precisions, plus the generic lowering
// through a QUnit.
#include "../csrc/qengine_cpu.hpp"
#include "../csrc/qfactory.hpp"
#include "../csrc/qunit.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace qrack_amd;

static void require(bool ok, const char* what)
{
    if (ok) return;
    std::fprintf(stderr, "adjoint_asan: %s\n", what);
    std::exit(1);
}

template <typename R> static std::vector<AdjointOp<R>> circuit(const std::vector<double>& theta)
{
    const R s2 = (R)0.70710678118654752440;
    std::vector<AdjointOp<R>> ops;
    auto rot = [&](std::vector<bitLenInt> qs, std::vector<Pauli> ps, double t, bool train = true) {
        AdjointOp<R> op;
        op.kind = AdjointOp<R>::Rotation;
        op.qubits = qs;
        op.paulis = ps;
        op.theta = t;
        op.trainable = train;
        ops.push_back(op);
    };
    rot({ 0 }, { PauliY }, theta[0]);
    rot({ 5 }, { PauliX }, theta[1]);
    rot({ 0, 5 }, { PauliX, PauliY }, theta[2]);
    AdjointOp<R> h;
    h.kind = AdjointOp<R>::Gate;
    h.qubits = { 2 };
    h.mtrx = { { s2, 0 }, { s2, 0 }, { s2, 0 }, { -s2, 0 } };
    h.controls = { 0 };
    ops.push_back(h);
    rot({ 1, 3 }, { PauliZ, PauliZ }, theta[3]);
    rot({ 4, 2 }, { PauliY, PauliZ }, 0.37, false);
    AdjointOp<R> sw; // a 2-qubit permutation with phases: unitary
    sw.kind = AdjointOp<R>::Gate;
    sw.qubits = { 3, 1 };
    sw.mtrx.assign(16, cplx<R>(0, 0));
    sw.mtrx[0 * 4 + 0] = { 1, 0 };
    sw.mtrx[1 * 4 + 2] = { 0, 1 };
    sw.mtrx[2 * 4 + 1] = { 0, 1 };
    sw.mtrx[3 * 4 + 3] = { 1, 0 };
    sw.anti = true;
    sw.controls = { 5 };
    ops.push_back(sw);
    rot({ 0, 1, 2, 3, 4, 5 }, { PauliX, PauliY, PauliZ, PauliX, PauliY, PauliZ }, theta[4]);
    rot({}, {}, theta[5]); // a global phase: its derivative is zero
    return ops;
}

template <typename R> static void battery(double tol)
{
    const bitLenInt n = 6;
    std::vector<PauliTerm> terms;
    for (bitLenInt b = 0; b + 1 < n; ++b) {
        terms.push_back({ 1.0, { b, (bitLenInt)(b + 1) }, { PauliX, PauliX } });
        terms.push_back({ 0.8, { b, (bitLenInt)(b + 1) }, { PauliY, PauliY } });
        terms.push_back({ 0.6, { b, (bitLenInt)(b + 1) }, { PauliZ, PauliZ } });
    }
    terms.push_back({ 0.25, {}, {} });
    terms.push_back({ -0.4, { 0, 3 }, { PauliY, PauliX } });
    const std::vector<double> theta{ 0.3, -0.2, 0.5, 0.7, -0.4, 0.9 };

    auto prepared = [&] {
        auto q = std::make_shared<QEngineCPU<R>>(n, 0u);
        q->SetPermutation(0b010101);
        q->H(1);
        q->CNOT(1, 4);
        return q;
    };
    auto energyAt = [&](const std::vector<double>& t) {
        auto q = prepared();
        std::vector<double> none;
        std::vector<AdjointOp<R>> ops = circuit<R>(t);
        for (AdjointOp<R>& op : ops) op.trainable = false;
        const double e = q->AdjointGradient(ops, terms, none);
        require(none.empty(), "untrainable ops left gradient entries");
        return e;
    };

    auto q = prepared();
    std::vector<cplx<R>> before(q->GetMaxQPower()), after(q->GetMaxQPower());
    q->GetQuantumState(before.data());
    std::vector<double> grad;
    const double e = q->AdjointGradient(circuit<R>(theta), terms, grad);
    require(grad.size() == theta.size(), "one entry per trainable rotation");
    require(std::fabs(e - energyAt(theta)) <= tol, "energy differs from the untrainable run");
    q->GetQuantumState(after.data());
    for (size_t i = 0; i < before.size(); ++i) {
        require(std::fabs((double)(before[i].re - after[i].re)) <= tol
                && std::fabs((double)(before[i].im - after[i].im)) <= tol,
            "the state did not come back");
    }
    // E is A + B cos 2t + C sin 2t in every angle: the shift by pi/4 is exact
    for (size_t k = 0; k < theta.size(); ++k) {
        std::vector<double> up = theta, down = theta;
        up[k] += M_PI / 4;
        down[k] -= M_PI / 4;
        require(std::fabs(grad[k] - (energyAt(up) - energyAt(down))) <= 4 * tol, "gradient entry");
    }
    require(std::fabs(grad.back()) <= tol, "a global phase has no derivative");

    // braket and H|psi>: <a|H|b> = conj <b|H|a>, <a|H|a> = E, <a|(H b)> = <a|H|b>
    auto a = prepared(), b = prepared(), d = prepared();
    a->RY((R)0.4, 2);
    b->RX((R)0.9, 5);
    const cplx<double> ab = b->PauliSumBraket(a, terms), ba = a->PauliSumBraket(b, terms);
    require(std::fabs(ab.re - ba.re) <= tol && std::fabs(ab.im + ba.im) <= tol, "braket is not Hermitian");
    const cplx<double> aa = a->PauliSumBraket(a, terms);
    require(std::fabs(aa.re - a->ExpectationPauliSum(terms)) <= tol && std::fabs(aa.im) <= tol, "<a|H|a>");
    b->PauliSumApplyInto(terms, d);
    const cplx<double> viaApply = d->PauliSumBraket(a, { PauliTerm{ 1.0, {}, {} } });
    require(std::fabs(viaApply.re - ab.re) <= tol && std::fabs(viaApply.im - ab.im) <= tol, "<a|(H b)>");
    bool threw = false;
    try {
        b->PauliSumApplyInto(terms, b);
    } catch (const QrackError&) {
        threw = true;
    }
    require(threw, "dest == this must throw");

    // generic lowering: a QUnit answers through host copies and stays as it was
    QInterfacePtr<R> u = CreateStack<R>(n, { "qunit", "cpu" }, 0u, 5, -1, 1);
    u->H(0);
    u->CNOT(0, 3);
    QInterfacePtr<R> ref = std::make_shared<QEngineCPU<R>>(n, 0u);
    ref->H(0);
    ref->CNOT(0, 3);
    std::vector<double> gu, gr;
    const double eu = u->AdjointGradient(circuit<R>(theta), terms, gu);
    const double er = ref->AdjointGradient(circuit<R>(theta), terms, gr);
    require(std::fabs(eu - er) <= tol && gu.size() == gr.size(), "generic lowering: energy");
    for (size_t k = 0; k < gu.size(); ++k) require(std::fabs(gu[k] - gr[k]) <= tol, "generic lowering: gradient");
    const cplx<double> uu = u->PauliSumBraket(u, terms);
    require(std::fabs(uu.re - u->ExpectationPauliSum(terms)) <= tol, "generic lowering: braket");
}

int main()
{
    battery<float>(2e-4);
    battery<double>(1e-11);
    std::printf("adjoint_asan OK\n");
    return 0;
}
