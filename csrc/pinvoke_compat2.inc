// pinvoke-compatible C ABI, part 2: measurement, swap family, Schmidt ops,
// boolean logic, QFT, ALU, separability/approximation setters, probability
// and expectation families, ket I/O, and the neuron/circuit delegates.
// (Included from pinvoke_compat.inc; same TU as capi.cpp.)

extern "C" {

// ---- measurement ------------------------------------------------------------

uintq M(uintq sid, uintq qv)
{
    uintq r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const bitLenInt t = mapq(s, qv);
        FOR_SIM(s, r = q.M(t) ? 1u : 0u);
    });
    return r;
}

uintq ForceM(uintq sid, uintq qv, bool r)
{
    uintq out = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const bitLenInt t = mapq(s, qv);
        FOR_SIM(s, out = q.ForceM(t, r, true) ? 1u : 0u);
    });
    return out;
}

uintq MAll(uintq sid)
{
    uintq r = 0;
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, r = (uintq)q.MAll()); });
    return r;
}

void MAllLong(uintq sid, uintq* r)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const bitLenInt nw = (s.Qubits() + 63u) / 64u;
        BigCap v{};
        FOR_SIM(s, v = q.MAllWide());
        for (bitLenInt w = 0; w < nw; ++w) r[w] = (w == 0) ? v.lo : ((w == 1) ? v.hi : 0u);
    });
}

uintq Measure(uintq sid, uintq n, int* b, uintq* qs)
{
    // joint (collapsing) Pauli-product measurement: rotate each listed
    // Pauli into Z, force-measure the parity, rotate back
    uintq r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<bitLenInt> tq;
        std::vector<int> tb;
        for (uintq i = 0; i < n; ++i) {
            if (b[i]) {
                tq.push_back(qv[i]);
                tb.push_back(b[i]);
            }
        }
        if (tb.empty()) return;
        // accumulate the parity onto the top listed qubit with a CNOT
        // chain, measure it (collapsing), uncompute — works on every layer
        FOR_SIM(s, ({
            pcToZ(q, (uintq)tb.size(), tb.data(), tq);
            const bitLenInt top = tq.back();
            for (size_t i = 0; i + 1 < tq.size(); ++i) q.CNOT(tq[i], top);
            r = q.M(top) ? 1u : 0u;
            for (size_t i = tq.size() - 1; i-- > 0;) q.CNOT(tq[i], top);
            pcRevert(q, (uintq)tb.size(), tb.data(), tq);
        }));
    });
    return r;
}

void MeasureShots(uintq sid, uintq n, uintq* qs, uintq shots, uintq* m)
{
    guarded((quid)sid, [&](SimSlot& s) {
        std::vector<bitCapInt> pows;
        for (uintq i = 0; i < n; ++i) pows.push_back(pow2(mapq(s, qs[i])));
        std::vector<unsigned long long> out((size_t)shots);
        FOR_SIM(s, q.MultiShotMeasureMask(pows, (unsigned)shots, out.data()));
        for (uintq i = 0; i < shots; ++i) m[i] = (uintq)out[i];
    });
}

// ---- swap family ------------------------------------------------------------

#define PC_GATE2(NAME, CALL)                                                                       \
    void NAME(uintq sid, uintq q1, uintq q2)                                                       \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            const bitLenInt a = mapq(s, q1), b2 = mapq(s, q2);                                     \
            FOR_SIM(s, q.CALL(a, b2));                                                             \
        });                                                                                        \
    }

PC_GATE2(SWAP, Swap)
PC_GATE2(ISWAP, ISwap)
PC_GATE2(AdjISWAP, IISwap)

void FSim(uintq sid, double theta, double phi, uintq q1, uintq q2)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const bitLenInt a = mapq(s, q1), b2 = mapq(s, q2);
        if (s.f) s.f->FSim((float)theta, (float)phi, a, b2);
        if (s.d) s.d->FSim(theta, phi, a, b2);
    });
}

void CSWAP(uintq sid, uintq n, uintq* c, uintq q1, uintq q2)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> cv = mapv(s, n, c);
        const bitLenInt a = mapq(s, q1), b2 = mapq(s, q2);
        FOR_SIM(s, q.CSwap(cv, a, b2));
    });
}

void ACSWAP(uintq sid, uintq n, uintq* c, uintq q1, uintq q2)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> cv = mapv(s, n, c);
        const bitLenInt a = mapq(s, q1), b2 = mapq(s, q2);
        FOR_SIM(s, q.AntiCSwap(cv, a, b2));
    });
}

// ---- Schmidt decomposition (compose/decompose/dispose) ----------------------

void Compose(uintq sid1, uintq sid2, uintq* qs)
{
    SimSlotPtr s1 = slot((quid)sid1);
    SimSlotPtr s2 = slot((quid)sid2);
    if (!s1 || !s2) return;
    std::lock_guard<std::mutex> lk1(s1->op);
    std::lock_guard<std::mutex> lk2(s2->op);
    try {
        const bitLenInt o = s1->Qubits();
        bitLenInt added = 0;
        if (s1->f && s2->f) {
            s1->f->Compose(s2->f->Clone());
            added = s1->Qubits() - o;
        } else if (s1->d && s2->d) {
            s1->d->Compose(s2->d->Clone());
            added = s1->Qubits() - o;
        } else {
            s1->error = 2;
            return;
        }
        if (qs) {
            // the caller names the new qubits: honor non-index ids by
            // switching to explicit mapping on demand
            bool needMap = s1->useQidMap;
            for (bitLenInt i = 0; !needMap && i < added; ++i) {
                if (qs[i] != (uintq)(o + i)) needMap = true;
            }
            if (needMap && !s1->useQidMap) {
                s1->useQidMap = true;
                s1->qidMap.clear();
                for (bitLenInt i = 0; i < o; ++i) s1->qidMap[(uint64_t)i] = i;
            }
            if (s1->useQidMap) {
                for (bitLenInt i = 0; i < added; ++i) s1->qidMap[(uint64_t)qs[i]] = o + i;
            }
        }
    } catch (const std::exception&) {
        s1->error = 1;
    }
}

uintq Decompose(uintq sid, uintq n, uintq* qs)
{
    quid nsid = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        SimSlotPtr ns = std::make_shared<SimSlot>();
        // split by clone: the clone disposes the complement, the original
        // disposes the listed register (both valid iff the split is
        // separable — the same precondition as the reference's Decompose)
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            const bitLenInt dst = s.Qubits() - (bitLenInt)n;
            ra.arrange(qv, dst);
            QInterfacePtr<float> dest = s.f->Clone();
            if (dst) dest->Dispose(0u, dst);
            s.f->Dispose(dst, (bitLenInt)n);
            ns->f = dest;
            ra.swaps.clear(); // decomposed qubits are gone; nothing to undo
        } else if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            const bitLenInt dst = s.Qubits() - (bitLenInt)n;
            ra.arrange(qv, dst);
            QInterfacePtr<double> dest = s.d->Clone();
            if (dst) dest->Dispose(0u, dst);
            s.d->Dispose(dst, (bitLenInt)n);
            ns->d = dest;
            ra.swaps.clear();
        }
        if (s.useQidMap) {
            for (uintq j = 0; j < n; ++j) {
                auto it = s.qidMap.find((uint64_t)qs[j]);
                if (it == s.qidMap.end()) continue;
                const bitLenInt oIdx = it->second;
                s.qidMap.erase(it);
                for (auto& kv : s.qidMap) {
                    if (kv.second > oIdx) --kv.second;
                }
            }
        }
        nsid = registerSlot(ns);
    });
    return (uintq)nsid;
}

void Dispose(uintq sid, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        const bitLenInt dst = s.Qubits() - (bitLenInt)n;
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            ra.arrange(qv, dst);
            s.f->Dispose(dst, (bitLenInt)n);
            ra.swaps.clear();
        } else if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            ra.arrange(qv, dst);
            s.d->Dispose(dst, (bitLenInt)n);
            ra.swaps.clear();
        }
        if (s.useQidMap) {
            for (uintq j = 0; j < n; ++j) {
                auto it = s.qidMap.find((uint64_t)qs[j]);
                if (it == s.qidMap.end()) continue;
                const bitLenInt oIdx = it->second;
                s.qidMap.erase(it);
                for (auto& kv : s.qidMap) {
                    if (kv.second > oIdx) --kv.second;
                }
            }
        }
    });
}

// ---- boolean logic ----------------------------------------------------------

#define PC_LOGIC(NAME, CALL)                                                                       \
    void NAME(uintq sid, uintq q1, uintq q2, uintq qo)                                             \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            const bitLenInt a = mapq(s, q1), b2 = mapq(s, q2), o = mapq(s, qo);                    \
            FOR_SIM(s, q.CALL(a, b2, o));                                                          \
        });                                                                                        \
    }

PC_LOGIC(AND, AND)
PC_LOGIC(OR, OR)
PC_LOGIC(XOR, XOR)
PC_LOGIC(NAND, NAND)
PC_LOGIC(NOR, NOR)
PC_LOGIC(XNOR, XNOR)

#define PC_CLLOGIC(NAME, CALL)                                                                     \
    void NAME(uintq sid, bool ci, uintq qi, uintq qo)                                              \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            const bitLenInt a = mapq(s, qi), o = mapq(s, qo);                                      \
            FOR_SIM(s, q.CALL(ci, a, o));                                                          \
        });                                                                                        \
    }

PC_CLLOGIC(CLAND, CLAND)
PC_CLLOGIC(CLOR, CLOR)
PC_CLLOGIC(CLXOR, CLXOR)
PC_CLLOGIC(CLNAND, CLNAND)
PC_CLLOGIC(CLNOR, CLNOR)
PC_CLLOGIC(CLXNOR, CLXNOR)

// ---- QFT --------------------------------------------------------------------

void QFT(uintq sid, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, q.QFTR(qv));
    });
}

void IQFT(uintq sid, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, q.IQFTR(qv));
    });
}

// ---- ALU --------------------------------------------------------------------

#define PC_WITH_REG1(sim, Rt, qv, BODY)                                                            \
    do {                                                                                           \
        RegArranger<QInterface<Rt>> ra(*(sim));                                                    \
        ra.arrange(qv, 0u);                                                                        \
        const bitLenInt start = 0u;                                                                \
        (void)start;                                                                               \
        BODY;                                                                                      \
    } while (0)

void ADD(uintq sid, uintq na, uintq* a, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) PC_WITH_REG1(s.f, float, qv, s.f->INC(av, 0u, (bitLenInt)n));
        if (s.d) PC_WITH_REG1(s.d, double, qv, s.d->INC(av, 0u, (bitLenInt)n));
    });
}

void SUB(uintq sid, uintq na, uintq* a, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) PC_WITH_REG1(s.f, float, qv, s.f->DEC(av, 0u, (bitLenInt)n));
        if (s.d) PC_WITH_REG1(s.d, double, qv, s.d->DEC(av, 0u, (bitLenInt)n));
    });
}

void ADDS(uintq sid, uintq na, uintq* a, uintq ov, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        std::vector<bitLenInt> qv = mapv(s, n, qs);
        qv.push_back(mapq(s, ov)); // overflow qubit rides just above
        if (s.f) PC_WITH_REG1(s.f, float, qv, s.f->INCS(av, 0u, (bitLenInt)n, (bitLenInt)n));
        if (s.d) PC_WITH_REG1(s.d, double, qv, s.d->INCS(av, 0u, (bitLenInt)n, (bitLenInt)n));
    });
}

void SUBS(uintq sid, uintq na, uintq* a, uintq ov, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        std::vector<bitLenInt> qv = mapv(s, n, qs);
        qv.push_back(mapq(s, ov));
        if (s.f) PC_WITH_REG1(s.f, float, qv, s.f->DECS(av, 0u, (bitLenInt)n, (bitLenInt)n));
        if (s.d) PC_WITH_REG1(s.d, double, qv, s.d->DECS(av, 0u, (bitLenInt)n, (bitLenInt)n));
    });
}

void MCADD(uintq sid, uintq na, uintq* a, uintq nc, uintq* c, uintq nq, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        const std::vector<bitLenInt> qv = mapv(s, nq, qs);
        const std::vector<bitLenInt> cv0 = mapv(s, nc, c);
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            ra.arrange(qv, 0u);
            std::vector<bitLenInt> cv;
            for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));
            s.f->CINC(av, 0u, (bitLenInt)nq, cv);
        }
        if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            ra.arrange(qv, 0u);
            std::vector<bitLenInt> cv;
            for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));
            s.d->CINC(av, 0u, (bitLenInt)nq, cv);
        }
    });
}

void MCSUB(uintq sid, uintq na, uintq* a, uintq nc, uintq* c, uintq nq, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        uint64_t av;
        if (!word1(s, na, a, av)) return;
        const std::vector<bitLenInt> qv = mapv(s, nq, qs);
        const std::vector<bitLenInt> cv0 = mapv(s, nc, c);
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            ra.arrange(qv, 0u);
            std::vector<bitLenInt> cv;
            for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));
            s.f->CDEC(av, 0u, (bitLenInt)nq, cv);
        }
        if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            ra.arrange(qv, 0u);
            std::vector<bitLenInt> cv;
            for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));
            s.d->CDEC(av, 0u, (bitLenInt)nq, cv);
        }
    });
}

// two-register ALU: arrange [q | o] contiguously at 0..2n-1
#define PC_ALU2(NAME, CALLF, CALLD)                                                                \
    void NAME(uintq sid, uintq na, uintq* a, uintq n, uintq* qs, uintq* os)                        \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            uint64_t av;                                                                           \
            if (!word1(s, na, a, av)) return;                                                      \
            std::vector<bitLenInt> all = mapv(s, n, qs);                                           \
            const std::vector<bitLenInt> ov = mapv(s, n, os);                                      \
            all.insert(all.end(), ov.begin(), ov.end());                                           \
            if (s.f) {                                                                             \
                RegArranger<QInterface<float>> ra(*s.f);                                           \
                ra.arrange(all, 0u);                                                               \
                s.f->CALLF;                                                                        \
            }                                                                                      \
            if (s.d) {                                                                             \
                RegArranger<QInterface<double>> ra(*s.d);                                          \
                ra.arrange(all, 0u);                                                               \
                s.d->CALLD;                                                                        \
            }                                                                                      \
        });                                                                                        \
    }

PC_ALU2(MUL, MUL(av, 0u, (bitLenInt)n, (bitLenInt)n), MUL(av, 0u, (bitLenInt)n, (bitLenInt)n))
PC_ALU2(DIV, DIV(av, 0u, (bitLenInt)n, (bitLenInt)n), DIV(av, 0u, (bitLenInt)n, (bitLenInt)n))

#define PC_ALU2M(NAME, CALLF, CALLD)                                                               \
    void NAME(uintq sid, uintq na, uintq* a, uintq* m, uintq n, uintq* qs, uintq* os)              \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            uint64_t av, mv;                                                                       \
            if (!word1(s, na, a, av) || !word1(s, na, m, mv)) return;                              \
            std::vector<bitLenInt> all = mapv(s, n, qs);                                           \
            const std::vector<bitLenInt> ov = mapv(s, n, os);                                      \
            all.insert(all.end(), ov.begin(), ov.end());                                           \
            if (s.f) {                                                                             \
                RegArranger<QInterface<float>> ra(*s.f);                                           \
                ra.arrange(all, 0u);                                                               \
                s.f->CALLF;                                                                        \
            }                                                                                      \
            if (s.d) {                                                                             \
                RegArranger<QInterface<double>> ra(*s.d);                                          \
                ra.arrange(all, 0u);                                                               \
                s.d->CALLD;                                                                        \
            }                                                                                      \
        });                                                                                        \
    }

PC_ALU2M(MULN, MULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n),
    MULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n))
PC_ALU2M(DIVN, IMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n),
    IMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n))
PC_ALU2M(POWN, POWModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n),
    POWModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n))

#define PC_ALU2C(NAME, CALLF, CALLD)                                                               \
    void NAME(uintq sid, uintq na, uintq* a, uintq nc, uintq* c, uintq n, uintq* qs, uintq* os)    \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            uint64_t av;                                                                           \
            if (!word1(s, na, a, av)) return;                                                      \
            std::vector<bitLenInt> all = mapv(s, n, qs);                                           \
            const std::vector<bitLenInt> ov = mapv(s, n, os);                                      \
            all.insert(all.end(), ov.begin(), ov.end());                                           \
            const std::vector<bitLenInt> cv0 = mapv(s, nc, c);                                     \
            if (s.f) {                                                                             \
                RegArranger<QInterface<float>> ra(*s.f);                                           \
                ra.arrange(all, 0u);                                                               \
                std::vector<bitLenInt> cv;                                                         \
                for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));                              \
                s.f->CALLF;                                                                        \
            }                                                                                      \
            if (s.d) {                                                                             \
                RegArranger<QInterface<double>> ra(*s.d);                                          \
                ra.arrange(all, 0u);                                                               \
                std::vector<bitLenInt> cv;                                                         \
                for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));                              \
                s.d->CALLD;                                                                        \
            }                                                                                      \
        });                                                                                        \
    }

PC_ALU2C(MCMUL, CMUL(av, 0u, (bitLenInt)n, (bitLenInt)n, cv),
    CMUL(av, 0u, (bitLenInt)n, (bitLenInt)n, cv))
PC_ALU2C(MCDIV, CDIV(av, 0u, (bitLenInt)n, (bitLenInt)n, cv),
    CDIV(av, 0u, (bitLenInt)n, (bitLenInt)n, cv))

#define PC_ALU2CM(NAME, CALLF, CALLD)                                                              \
    void NAME(uintq sid, uintq na, uintq* a, uintq nc, uintq* c, uintq* m, uintq n, uintq* qs,     \
        uintq* os)                                                                                 \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            uint64_t av, mv;                                                                       \
            if (!word1(s, na, a, av) || !word1(s, na, m, mv)) return;                              \
            std::vector<bitLenInt> all = mapv(s, n, qs);                                           \
            const std::vector<bitLenInt> ov = mapv(s, n, os);                                      \
            all.insert(all.end(), ov.begin(), ov.end());                                           \
            const std::vector<bitLenInt> cv0 = mapv(s, nc, c);                                     \
            if (s.f) {                                                                             \
                RegArranger<QInterface<float>> ra(*s.f);                                           \
                ra.arrange(all, 0u);                                                               \
                std::vector<bitLenInt> cv;                                                         \
                for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));                              \
                s.f->CALLF;                                                                        \
            }                                                                                      \
            if (s.d) {                                                                             \
                RegArranger<QInterface<double>> ra(*s.d);                                          \
                ra.arrange(all, 0u);                                                               \
                std::vector<bitLenInt> cv;                                                         \
                for (bitLenInt ci : cv0) cv.push_back(ra.locate(ci));                              \
                s.d->CALLD;                                                                        \
            }                                                                                      \
        });                                                                                        \
    }

PC_ALU2CM(MCMULN, CMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv),
    CMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv))
PC_ALU2CM(MCDIVN, CIMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv),
    CIMULModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv))
PC_ALU2CM(MCPOWN, CPOWModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv),
    CPOWModNOut(av, mv, 0u, (bitLenInt)n, (bitLenInt)n, cv))

void LDA(uintq sid, uintq ni, uintq* qi, uintq nv, uintq* qv2, unsigned char* t)
{
    guarded((quid)sid, [&](SimSlot& s) {
        std::vector<bitLenInt> all = mapv(s, ni, qi);
        const std::vector<bitLenInt> vv = mapv(s, nv, qv2);
        all.insert(all.end(), vv.begin(), vv.end());
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            ra.arrange(all, 0u);
            s.f->IndexedLDA(0u, (bitLenInt)ni, (bitLenInt)ni, (bitLenInt)nv, t, true);
        }
        if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            ra.arrange(all, 0u);
            s.d->IndexedLDA(0u, (bitLenInt)ni, (bitLenInt)ni, (bitLenInt)nv, t, true);
        }
    });
}

#define PC_IDXC(NAME, CALL)                                                                        \
    void NAME(uintq sid, uintq cq, uintq ni, uintq* qi, uintq nv, uintq* qv2, unsigned char* t)    \
    {                                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            std::vector<bitLenInt> all = mapv(s, ni, qi);                                          \
            const std::vector<bitLenInt> vv = mapv(s, nv, qv2);                                    \
            all.insert(all.end(), vv.begin(), vv.end());                                           \
            all.push_back(mapq(s, cq));                                                            \
            if (s.f) {                                                                             \
                RegArranger<QInterface<float>> ra(*s.f);                                           \
                ra.arrange(all, 0u);                                                               \
                s.f->CALL(                                                                         \
                    0u, (bitLenInt)ni, (bitLenInt)ni, (bitLenInt)nv, (bitLenInt)(ni + nv), t);     \
            }                                                                                      \
            if (s.d) {                                                                             \
                RegArranger<QInterface<double>> ra(*s.d);                                          \
                ra.arrange(all, 0u);                                                               \
                s.d->CALL(                                                                         \
                    0u, (bitLenInt)ni, (bitLenInt)ni, (bitLenInt)nv, (bitLenInt)(ni + nv), t);     \
            }                                                                                      \
        });                                                                                        \
    }

PC_IDXC(ADC, IndexedADC)
PC_IDXC(SBC, IndexedSBC)

void Hash(uintq sid, uintq n, uintq* qs, unsigned char* t)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) {
            RegArranger<QInterface<float>> ra(*s.f);
            ra.arrange(qv, 0u);
            s.f->Hash(0u, (bitLenInt)n, t);
        }
        if (s.d) {
            RegArranger<QInterface<double>> ra(*s.d);
            ra.arrange(qv, 0u);
            s.d->Hash(0u, (bitLenInt)n, t);
        }
    });
}

// ---- separability / fidelity / approximation --------------------------------

bool TrySeparate1Qb(uintq sid, uintq q1)
{
    return qrack_try_separate_1qb((quid)sid, (uint64_t)q1) != 0;
}

bool TrySeparate2Qb(uintq sid, uintq q1, uintq q2)
{
    return qrack_try_separate_2qb((quid)sid, (uint64_t)q1, (uint64_t)q2) != 0;
}

bool TrySeparateTol(uintq sid, uintq n, uintq* qs, double tol)
{
    bool r = false;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, r = q.TrySeparate(qv, (decltype(q.Prob(0)))tol));
    });
    return r;
}

void Separate(uintq sid, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, (void)q.TrySeparate(qv, (decltype(q.Prob(0)))0.0));
    });
}

bool AreFactorized(uintq sid, uintq n1, uintq* a, uintq n2, uintq* b, bool fc)
{
    (void)fc;
    bool r = false;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> av = mapv(s, n1, a);
        const std::vector<bitLenInt> bv = mapv(s, n2, b);
        FOR_SIM(s, r = q.AreFactorized(av, bv));
    });
    return r;
}

double GetUnitaryFidelity(uintq sid) { return qrack_get_unitary_fidelity((quid)sid); }
void ResetUnitaryFidelity(uintq sid) { qrack_reset_unitary_fidelity((quid)sid); }
void SetSdrp(uintq sid, double sdrp) { qrack_set_sdrp((quid)sid, sdrp); }
void SetNcrp(uintq sid, double ncrp) { qrack_set_ncrp((quid)sid, ncrp); }

void SetSprp(uintq sid, double sprp)
{
    (void)sid;
    (void)sprp; // stabilizer phase rounding: covered by SetNcrp in this build
}

void SetReactiveSeparate(uintq sid, bool irs)
{
    qrack_set_reactive_separate((quid)sid, irs ? 1 : 0);
}

void SetTInjection(uintq sid, bool iti)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.SetTInjection(iti)); });
}

void SetUseExactNearClifford(uintq sid, bool enc)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.SetUseExactNearClifford(enc)); });
}

void SetNoiseParameter(uintq sid, double np)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.SetNoiseParameter(np)); });
}

void SetAceMaxQb(uintq sid, uintq qb) { qrack_set_ace_max_qb((quid)sid, (uint64_t)qb); }

void SetSparseAceMaxMb(uintq sid, size_t mb)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.SetSparseAceMaxMb((uint64_t)mb)); });
}

void SetStochastic(uintq sid, bool st)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.SetStochastic(st)); });
}

void Normalize(uintq sid)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, q.NormalizeState()); });
}

// ---- probability / expectation families -------------------------------------

double Prob(uintq sid, uintq qv)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const bitLenInt t = mapq(s, qv);
        FOR_SIM(s, r = (double)q.Prob(t));
    });
    return r;
}

double ProbRdm(uintq sid, uintq qv) { return Prob(sid, qv); }

void HighestProbAll(uintq sid, uintq* r)
{
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, *r = (uintq)q.HighestProbAll()); });
}

void HighestProbAllN(uintq sid, uintq n, uintq* r)
{
    guarded((quid)sid, [&](SimSlot& s) {
        bitCapInt v = 0;
        FOR_SIM(s, v = q.HighestProbAll());
        for (uintq w = 0; w < n; ++w) r[w] = (w == 0) ? (uintq)v : 0u;
    });
}

void ProbAll(uintq sid, uintq n, uintq* qs, real1_s* p)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<double> joint(((size_t)1) << n);
        FOR_SIM(s, q.ProbBitsAll(qv, joint.data()));
        for (size_t i = 0; i < joint.size(); ++i) p[i] = (real1_s)joint[i];
    });
}

double PermutationProb(uintq sid, uintq n, uintq* qs, bool* c)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        bitCapInt mask = 0, perm = 0;
        for (uintq i = 0; i < n; ++i) {
            const bitCapInt p = pow2(mapq(s, qs[i]));
            mask |= p;
            if (c[i]) perm |= p;
        }
        FOR_SIM(s, r = (double)q.ProbMask(mask, perm));
    });
    return r;
}

double PermutationProbRdm(uintq sid, uintq n, uintq* qs, bool* c, bool r)
{
    (void)r;
    return PermutationProb(sid, n, qs, c);
}

double PermutationExpectation(uintq sid, uintq n, uintq* qs)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, r = q.ExpectationBitsAll(qv));
    });
    return r;
}

double PermutationExpectationRdm(uintq sid, uintq n, uintq* qs, bool r)
{
    double out = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, out = q.ExpectationBitsAllRdm(r, qv));
    });
    return out;
}

double Variance(uintq sid, uintq n, uintq* qs)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        FOR_SIM(s, r = q.VarianceBitsAll(qv));
    });
    return r;
}

double VarianceRdm(uintq sid, uintq n, uintq* qs, bool r)
{
    (void)r;
    return Variance(sid, n, qs);
}

// the reference's Factorized functions take TWO perms/weights per bit
static std::vector<double> pcPairWeights(uintq n, const uintq* c)
{
    std::vector<double> w;
    for (uintq i = 0; i < 2u * n; ++i) w.push_back((double)c[i]);
    return w;
}

double FactorizedExpectation(uintq sid, uintq n, uintq* qs, uintq m, uintq* c)
{
    (void)m; // words per perm; single-word values only
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        const std::vector<double> w = pcPairWeights(n, c);
        FOR_SIM(s, r = q.ExpectationFloatsFactorized(qv, w));
    });
    return r;
}

double FactorizedExpectationRdm(uintq sid, uintq n, uintq* qs, uintq m, uintq* c, bool r)
{
    (void)r;
    return FactorizedExpectation(sid, n, qs, m, c);
}

double FactorizedVariance(uintq sid, uintq n, uintq* qs, uintq m, uintq* c)
{
    (void)m;
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        const std::vector<double> w = pcPairWeights(n, c);
        FOR_SIM(s, r = q.VarianceFloatsFactorized(qv, w));
    });
    return r;
}

double FactorizedVarianceRdm(uintq sid, uintq n, uintq* qs, uintq m, uintq* c, bool r)
{
    (void)r;
    return FactorizedVariance(sid, n, qs, m, c);
}

double FactorizedExpectationFp(uintq sid, uintq n, uintq* qs, real1_s* c)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<double> w;
        for (uintq i = 0; i < 2u * n; ++i) w.push_back((double)c[i]);
        FOR_SIM(s, r = q.ExpectationFloatsFactorized(qv, w));
    });
    return r;
}

double FactorizedExpectationFpRdm(uintq sid, uintq n, uintq* qs, real1_s* c, bool r)
{
    (void)r;
    return FactorizedExpectationFp(sid, n, qs, c);
}

double FactorizedVarianceFp(uintq sid, uintq n, uintq* qs, real1_s* c)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<double> w;
        for (uintq i = 0; i < 2u * n; ++i) w.push_back((double)c[i]);
        FOR_SIM(s, r = q.VarianceFloatsFactorized(qv, w));
    });
    return r;
}

double FactorizedVarianceFpRdm(uintq sid, uintq n, uintq* qs, real1_s* c, bool r)
{
    (void)r;
    return FactorizedVarianceFp(sid, n, qs, c);
}

// basis given as (z, x, y) triplet per qubit in the reference convention:
// the 2x2 basis-change op columns; here b holds 3 reals per qubit that
// define the rotation U with U|0> the +1 eigenvector (theta, phi, lambda)
double UnitaryExpectation(uintq sid, uintq n, uintq* qs, real1_s* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) {
            std::vector<cplx<float>> ops;
            for (uintq i = 0; i < n; ++i) {
                cplx<float> m[4];
                pcU4<float>(m, (double)b[3 * i], (double)b[3 * i + 1], (double)b[3 * i + 2], 0.0);
                for (int e = 0; e < 4; ++e) ops.push_back(m[e]);
            }
            r = s.f->ExpectationUnitaryAll(qv, ops);
        }
        if (s.d) {
            std::vector<cplx<double>> ops;
            for (uintq i = 0; i < n; ++i) {
                cplx<double> m[4];
                pcU4<double>(m, (double)b[3 * i], (double)b[3 * i + 1], (double)b[3 * i + 2], 0.0);
                for (int e = 0; e < 4; ++e) ops.push_back(m[e]);
            }
            r = s.d->ExpectationUnitaryAll(qv, ops);
        }
    });
    return r;
}

double MatrixExpectation(uintq sid, uintq n, uintq* qs, real1_s* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) {
            std::vector<cplx<float>> ops;
            for (uintq i = 0; i < 8u * n; i += 2)
                ops.push_back(cplx<float>((float)b[i], (float)b[i + 1]));
            r = s.f->ExpectationUnitaryAll(qv, ops);
        }
        if (s.d) {
            std::vector<cplx<double>> ops;
            for (uintq i = 0; i < 8u * n; i += 2)
                ops.push_back(cplx<double>((double)b[i], (double)b[i + 1]));
            r = s.d->ExpectationUnitaryAll(qv, ops);
        }
    });
    return r;
}

#define PC_EIG(NAME, METHOD, PACK8)                                                                \
    double NAME(uintq sid, uintq n, uintq* qs, real1_s* b, real1_s* e)                             \
    {                                                                                              \
        double r = 0;                                                                              \
        guarded((quid)sid, [&](SimSlot& s) {                                                       \
            const std::vector<bitLenInt> qv = mapv(s, n, qs);                                      \
            std::vector<double> eig;                                                               \
            for (uintq i = 0; i < 2u * n; ++i) eig.push_back((double)e[i]);                        \
            if (s.f) {                                                                             \
                std::vector<cplx<float>> ops;                                                      \
                if (PACK8) {                                                                       \
                    for (uintq i = 0; i < 8u * n; i += 2)                                          \
                        ops.push_back(cplx<float>((float)b[i], (float)b[i + 1]));                  \
                } else {                                                                           \
                    for (uintq i = 0; i < n; ++i) {                                                \
                        cplx<float> m[4];                                                          \
                        pcU4<float>(m, (double)b[3 * i], (double)b[3 * i + 1],                     \
                            (double)b[3 * i + 2], 0.0);                                            \
                        for (int ee = 0; ee < 4; ++ee) ops.push_back(m[ee]);                       \
                    }                                                                              \
                }                                                                                  \
                r = s.f->METHOD(qv, ops, eig);                                                     \
            }                                                                                      \
            if (s.d) {                                                                             \
                std::vector<cplx<double>> ops;                                                     \
                if (PACK8) {                                                                       \
                    for (uintq i = 0; i < 8u * n; i += 2)                                          \
                        ops.push_back(cplx<double>((double)b[i], (double)b[i + 1]));               \
                } else {                                                                           \
                    for (uintq i = 0; i < n; ++i) {                                                \
                        cplx<double> m[4];                                                         \
                        pcU4<double>(m, (double)b[3 * i], (double)b[3 * i + 1],                    \
                            (double)b[3 * i + 2], 0.0);                                            \
                        for (int ee = 0; ee < 4; ++ee) ops.push_back(m[ee]);                       \
                    }                                                                              \
                }                                                                                  \
                r = s.d->METHOD(qv, ops, eig);                                                     \
            }                                                                                      \
        });                                                                                        \
        return r;                                                                                  \
    }

PC_EIG(UnitaryExpectationEigenVal, ExpectationUnitaryAll, 0)
PC_EIG(MatrixExpectationEigenVal, ExpectationUnitaryAll, 1)
PC_EIG(UnitaryVarianceEigenVal, VarianceUnitaryAll, 0)
PC_EIG(MatrixVarianceEigenVal, VarianceUnitaryAll, 1)

double UnitaryVariance(uintq sid, uintq n, uintq* qs, real1_s* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) {
            std::vector<cplx<float>> ops;
            for (uintq i = 0; i < n; ++i) {
                cplx<float> m[4];
                pcU4<float>(m, (double)b[3 * i], (double)b[3 * i + 1], (double)b[3 * i + 2], 0.0);
                for (int e = 0; e < 4; ++e) ops.push_back(m[e]);
            }
            r = s.f->VarianceUnitaryAll(qv, ops);
        }
        if (s.d) {
            std::vector<cplx<double>> ops;
            for (uintq i = 0; i < n; ++i) {
                cplx<double> m[4];
                pcU4<double>(m, (double)b[3 * i], (double)b[3 * i + 1], (double)b[3 * i + 2], 0.0);
                for (int e = 0; e < 4; ++e) ops.push_back(m[e]);
            }
            r = s.d->VarianceUnitaryAll(qv, ops);
        }
    });
    return r;
}

double MatrixVariance(uintq sid, uintq n, uintq* qs, real1_s* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (s.f) {
            std::vector<cplx<float>> ops;
            for (uintq i = 0; i < 8u * n; i += 2)
                ops.push_back(cplx<float>((float)b[i], (float)b[i + 1]));
            r = s.f->VarianceUnitaryAll(qv, ops);
        }
        if (s.d) {
            std::vector<cplx<double>> ops;
            for (uintq i = 0; i < 8u * n; i += 2)
                ops.push_back(cplx<double>((double)b[i], (double)b[i + 1]));
            r = s.d->VarianceUnitaryAll(qv, ops);
        }
    });
    return r;
}

double PauliExpectation(uintq sid, uintq n, uintq* qs, uintq* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<Pauli> ps;
        for (uintq i = 0; i < n; ++i) ps.push_back((Pauli)b[i]);
        FOR_SIM(s, r = q.ExpectationPauliAll(qv, ps));
    });
    return r;
}

double PauliVariance(uintq sid, uintq n, uintq* qs, uintq* b)
{
    double r = 0;
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        std::vector<Pauli> ps;
        for (uintq i = 0; i < n; ++i) ps.push_back((Pauli)b[i]);
        FOR_SIM(s, r = q.VariancePauliAll(qv, ps));
    });
    return r;
}

double JointEnsembleProbability(uintq sid, uintq n, int* b, uintq* qs)
{
    std::vector<uint64_t> qq(qs, qs + n);
    return qrack_joint_ensemble_probability((quid)sid, b, qq.data(), n);
}

// ---- ket / probability I/O and dumps ----------------------------------------

void InKet(uintq sid, real1_s* ket)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const bitCapInt np = pow2(s.Qubits());
        if (s.f) {
            std::vector<cplx<float>> sv((size_t)np);
            for (bitCapInt i = 0; i < np; ++i)
                sv[(size_t)i] = cplx<float>(ket[2 * (size_t)i], ket[2 * (size_t)i + 1]);
            s.f->SetQuantumState(sv.data());
        }
        if (s.d) {
            std::vector<cplx<double>> sv((size_t)np);
            for (bitCapInt i = 0; i < np; ++i)
                sv[(size_t)i] = cplx<double>(ket[2 * (size_t)i], ket[2 * (size_t)i + 1]);
            s.d->SetQuantumState(sv.data());
        }
    });
}

void OutKet(uintq sid, real1_s* ket)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const bitCapInt np = pow2(s.Qubits());
        if (s.f) {
            std::vector<cplx<float>> sv((size_t)np);
            s.f->GetQuantumState(sv.data());
            for (bitCapInt i = 0; i < np; ++i) {
                ket[2 * (size_t)i] = (real1_s)sv[(size_t)i].re;
                ket[2 * (size_t)i + 1] = (real1_s)sv[(size_t)i].im;
            }
        }
        if (s.d) {
            std::vector<cplx<double>> sv((size_t)np);
            s.d->GetQuantumState(sv.data());
            for (bitCapInt i = 0; i < np; ++i) {
                ket[2 * (size_t)i] = (real1_s)sv[(size_t)i].re;
                ket[2 * (size_t)i + 1] = (real1_s)sv[(size_t)i].im;
            }
        }
    });
}

void OutProbs(uintq sid, real1_s* p)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const bitCapInt np = pow2(s.Qubits());
        if (s.f) {
            std::vector<float> pr((size_t)np);
            s.f->GetProbs(pr.data());
            for (bitCapInt i = 0; i < np; ++i) p[(size_t)i] = (real1_s)pr[(size_t)i];
        }
        if (s.d) {
            std::vector<double> pr((size_t)np);
            s.d->GetProbs(pr.data());
            for (bitCapInt i = 0; i < np; ++i) p[(size_t)i] = (real1_s)pr[(size_t)i];
        }
    });
}

void OutReducedDensityMatrix(uintq sid, uintq n, uintq* qs, real1_s* rdm)
{
    guarded((quid)sid, [&](SimSlot& s) {
        const std::vector<bitLenInt> qv = mapv(s, n, qs);
        if (n > 12u) {
            s.error = 2;
            return;
        }
        std::vector<cplx<double>> m(((size_t)1 << n) << n);
        try {
            if (s.f) s.f->GetReducedDensityMatrix(qv, m.data());
            if (s.d) s.d->GetReducedDensityMatrix(qv, m.data());
        } catch (const QrackError&) {
            // the width cap of the generic lowering keeps its error code
            if (s.Qubits() <= 26u) throw;
            s.error = 2;
            return;
        }
        for (size_t k = 0; k < m.size(); ++k) {
            rdm[2 * k] = (real1_s)m[k].re;
            rdm[2 * k + 1] = (real1_s)m[k].im;
        }
    });
}

void DumpIds(uintq sid, IdCallback callback)
{
    SimSlotPtr s = slot((quid)sid);
    if (!s || !callback) return;
    std::lock_guard<std::mutex> lk(s->op);
    if (s->useQidMap) {
        for (const auto& kv : s->qidMap) callback((uintq)kv.first);
    } else {
        for (bitLenInt i = 0; i < s->Qubits(); ++i) callback((uintq)i);
    }
}

void Dump(uintq sid, ProbAmpCallback callback)
{
    SimSlotPtr sp = slot((quid)sid);
    if (!sp || !callback) return;
    std::lock_guard<std::mutex> lk(sp->op);
    SimSlot& s = *sp;
    const bitCapInt np = pow2(s.Qubits());
    if (s.f) {
        std::vector<cplx<float>> sv((size_t)np);
        s.f->GetQuantumState(sv.data());
        for (bitCapInt i = 0; i < np; ++i) {
            if (!callback((size_t)i, (double)sv[(size_t)i].re, (double)sv[(size_t)i].im)) break;
        }
    } else if (s.d) {
        std::vector<cplx<double>> sv((size_t)np);
        s.d->GetQuantumState(sv.data());
        for (bitCapInt i = 0; i < np; ++i) {
            if (!callback((size_t)i, sv[(size_t)i].re, sv[(size_t)i].im)) break;
        }
    }
}

size_t random_choice(uintq sid, size_t n, double* p)
{
    double r = 0.5;
    guarded((quid)sid, [&](SimSlot& s) { FOR_SIM(s, r = (double)q.Rand()); });
    double acc = 0;
    for (size_t i = 0; i < n; ++i) {
        acc += p[i];
        if (r < acc) return i;
    }
    return n ? (n - 1) : 0;
}

void PhaseParity(uintq sid, double lambda, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        bitCapInt mask = 0;
        for (uintq i = 0; i < n; ++i) mask |= pow2(mapq(s, qs[i]));
        if (s.f) s.f->PhaseParity((float)lambda, mask);
        if (s.d) s.d->PhaseParity(lambda, mask);
    });
}

void PhaseRootN(uintq sid, uintq p, uintq n, uintq* qs)
{
    guarded((quid)sid, [&](SimSlot& s) {
        for (uintq i = 0; i < n; ++i) {
            const bitLenInt t = mapq(s, qs[i]);
            FOR_SIM(s, q.PhaseRootN((bitLenInt)p, t));
        }
    });
}

// ---- neuron / circuit delegates (same handle spaces as qrack_*) -------------

uintq init_qneuron(uintq sid, uintq n, uintq* c, uintq qv)
{
    std::vector<uint64_t> cc(c, c + n);
    return (uintq)qrack_init_qneuron((quid)sid, cc.data(), n, (uint64_t)qv, 0, 1.0, 1e-6);
}

uintq clone_qneuron(uintq nid)
{
    (void)nid; // neuron cloning is not supported in this build
    return 0;
}
void destroy_qneuron(uintq nid) { qrack_destroy_qneuron((quid)nid); }

void set_qneuron_angles(uintq nid, real1_s* angles)
{
    const uint64_t n = 1ull << qrack_get_qneuron_qubit_count((quid)nid);
    std::vector<double> a(n);
    for (uint64_t i = 0; i < n; ++i) a[i] = (double)angles[i];
    qrack_set_qneuron_angles((quid)nid, a.data(), n);
}

void get_qneuron_angles(uintq nid, real1_s* angles)
{
    const uint64_t n = 1ull << qrack_get_qneuron_qubit_count((quid)nid);
    std::vector<double> a(n);
    qrack_get_qneuron_angles((quid)nid, a.data(), n);
    for (uint64_t i = 0; i < n; ++i) angles[i] = (real1_s)a[i];
}

double qneuron_predict(uintq nid, real1_s* angles, bool e, bool r, uintq f, double a)
{
    (void)angles;
    qrack_set_qneuron_activation_fn((quid)nid, (int)f);
    qrack_set_qneuron_alpha((quid)nid, a);
    return qrack_qneuron_predict((quid)nid, e ? 1 : 0, r ? 1 : 0);
}

double qneuron_unpredict(uintq nid, real1_s* angles, bool e, uintq f, double a)
{
    (void)angles;
    qrack_set_qneuron_activation_fn((quid)nid, (int)f);
    qrack_set_qneuron_alpha((quid)nid, a);
    return qrack_qneuron_unpredict((quid)nid, e ? 1 : 0);
}

double qneuron_learn_cycle(uintq nid, real1_s* angles, bool e, uintq f, double a)
{
    (void)angles;
    qrack_set_qneuron_activation_fn((quid)nid, (int)f);
    qrack_set_qneuron_alpha((quid)nid, a);
    qrack_qneuron_learn_cycle((quid)nid, 0.5, e ? 1 : 0);
    return qrack_qneuron_predict((quid)nid, e ? 1 : 0, 0);
}

void qneuron_learn(uintq nid, real1_s* angles, double eta, bool e, bool r, uintq f, double a)
{
    (void)angles;
    qrack_set_qneuron_activation_fn((quid)nid, (int)f);
    qrack_set_qneuron_alpha((quid)nid, a);
    qrack_qneuron_learn((quid)nid, eta, e ? 1 : 0, r ? 1 : 0);
}

void set_qneuron_sim(uintq nid, uintq sid, uintq n, uintq* c, uintq qv)
{
    (void)nid;
    (void)sid;
    (void)n;
    (void)c;
    (void)qv; // re-binding a neuron to a new simulator is not supported
}

void qneuron_learn_permutation(
    uintq nid, real1_s* angles, double eta, bool e, bool r, uintq f, double a)
{
    (void)angles;
    (void)r;
    qrack_set_qneuron_activation_fn((quid)nid, (int)f);
    qrack_set_qneuron_alpha((quid)nid, a);
    qrack_qneuron_learn_permutation((quid)nid, eta, e ? 1 : 0, 0u);
}

uintq init_qcircuit(bool collapse, bool clifford)
{
    (void)collapse;
    (void)clifford;
    return (uintq)qrack_init_qcircuit(0u);
}

uintq init_qcircuit_clone(uintq cid)
{
    // clone by inverse-of-inverse (both are fresh circuit handles)
    const quid inv = qrack_qcircuit_inverse((quid)cid);
    const quid clone = qrack_qcircuit_inverse(inv);
    qrack_destroy_qcircuit(inv);
    return (uintq)clone;
}
void destroy_qcircuit(uintq cid) { qrack_destroy_qcircuit((quid)cid); }
uintq get_qcircuit_qubit_count(uintq cid) { return qrack_qcircuit_qubit_count((quid)cid); }
uintq qcircuit_inverse(uintq cid) { return (uintq)qrack_qcircuit_inverse((quid)cid); }
uintq qcircuit_past_light_cone(uintq cid, uintq n, uintq* qs)
{
    std::vector<uint64_t> qq(qs, qs + n);
    return (uintq)qrack_qcircuit_past_light_cone((quid)cid, qq.data(), n);
}
void qcircuit_swap(uintq cid, uintq q1, uintq q2)
{
    qrack_qcircuit_swap((quid)cid, (uint64_t)q1, (uint64_t)q2);
}
void qcircuit_append_1qb(uintq cid, double* m, uintq qv)
{
    qrack_qcircuit_append_1qb((quid)cid, m, (uint64_t)qv);
}
void qcircuit_append_mc(uintq cid, double* m, uintq n, uintq* c, uintq qv, uintq p)
{
    std::vector<uint64_t> cc(c, c + n);
    qrack_qcircuit_append_mc((quid)cid, m, cc.data(), n, (uint64_t)qv, (uint64_t)p);
}
void qcircuit_run(uintq cid, uintq sid) { qrack_qcircuit_run((quid)cid, (quid)sid); }
void qcircuit_out_to_file(uintq cid, char* f) { qrack_qcircuit_out_to_file((quid)cid, f); }
void qcircuit_in_from_file(uintq cid, char* f)
{
    // the reference loads INTO the existing handle: load via the native
    // path (which registers a fresh handle), then move the circuit
    // contents into the caller's slot and drop the temporary
    const quid tmp = qrack_qcircuit_in_from_file(f);
    CircSlotPtr dst = circSlot((quid)cid);
    CircSlotPtr src = circSlot(tmp);
    if (dst && src) {
        std::lock_guard<std::mutex> lk(dst->op);
        dst->f = src->f;
        dst->d = src->d;
    }
    qrack_destroy_qcircuit(tmp);
}
size_t qcircuit_out_to_string_length(uintq cid)
{
    return qrack_qcircuit_out_to_string_length((quid)cid);
}
void qcircuit_out_to_string(uintq cid, char* f)
{
    const uint64_t cap = qrack_qcircuit_out_to_string_length((quid)cid) + 1u;
    qrack_qcircuit_out_to_string((quid)cid, f, cap);
}


// ---- TimeEvolve and quadrant stubs ------------------------------------------

struct _QrackTimeEvolveOpHeader {
    unsigned target;
    unsigned controlLen;
    unsigned controls[32u];
};

void TimeEvolve(uintq sid, double t, uintq n, _QrackTimeEvolveOpHeader* teos, uintq mn,
    double* mtrx)
{
    (void)mn;
    guarded((quid)sid, [&](SimSlot& s) {
        size_t off = 0;
        if (s.f) {
            std::vector<HamiltonianOp<float>> h;
            for (uintq i = 0; i < n; ++i) {
                HamiltonianOp<float> op;
                op.target = mapq(s, teos[i].target);
                for (unsigned c = 0; c < teos[i].controlLen; ++c)
                    op.controls.push_back(mapq(s, teos[i].controls[c]));
                op.uniform = teos[i].controlLen > 0;
                const size_t mats = ((size_t)1) << teos[i].controlLen;
                for (size_t e = 0; e < 4u * mats; ++e) {
                    op.matrix.push_back(
                        cplx<float>((float)mtrx[off + 2 * e], (float)mtrx[off + 2 * e + 1]));
                }
                off += 8u * mats;
                h.push_back(op);
            }
            s.f->TimeEvolve(h, (float)t);
        }
        if (s.d) {
            std::vector<HamiltonianOp<double>> h;
            for (uintq i = 0; i < n; ++i) {
                HamiltonianOp<double> op;
                op.target = mapq(s, teos[i].target);
                for (unsigned c = 0; c < teos[i].controlLen; ++c)
                    op.controls.push_back(mapq(s, teos[i].controls[c]));
                op.uniform = teos[i].controlLen > 0;
                const size_t mats = ((size_t)1) << teos[i].controlLen;
                for (size_t e = 0; e < 4u * mats; ++e) {
                    op.matrix.push_back(cplx<double>(mtrx[off + 2 * e], mtrx[off + 2 * e + 1]));
                }
                off += 8u * mats;
                h.push_back(op);
            }
            s.d->TimeEvolve(h, t);
        }
    });
}

// quadrant hints are empty virtuals on the reference QInterface too
// (/root/reference/include/qinterface.hpp:3040-3048)
void SetMajorQuadrant(uintq sid, bool qb)
{
    (void)sid;
    (void)qb;
}
void SetQuadrant(uintq sid, uintq t, bool b)
{
    (void)sid;
    (void)t;
    (void)b;
}
void FlipQuadrant(uintq sid, uintq t)
{
    (void)sid;
    (void)t;
}

} // extern "C"
