"""Expected values for the HPS family of BFV multiplication (HPS, HPSPOVERQ, HPSPOVERQLEVELED): TEST infrastructure.

  tables()    : every table of CryptoParametersBFVRNS::PrecomputeCRTTables' HPS block (bfvrns-cryptoparameters.cpp:143-665) from
                PYTHON INTEGERS by the reference's own formulas (big products, floor divisions), in the layout of fhe_hps_table;
  eval_mult() : LeveledSHEBFVRNS::EvalMult (bfvrns-leveledshe.cpp:198-439) composed from the oracle's members
                (orc_switch_crt_basis, orc_fast_expand_crt_basis_p_over_q, orc_scale_and_round, orc_expand_crt_basis_ql_hat,
                orc_ntt_*_tower) with those tables.  test_hps_host.py pins it against the live reference.
"""
import numpy as np

import libs

HPS, HPSPOVERQ, HPSPOVERQLEVELED = 1, 2, 3
MASK = (1 << 64) - 1


def prod(v):
    p = 1
    for x in v:
        p *= int(x)
    return p


def mu128(mods):
    return np.array([[((1 << 128) // int(d)) & MASK, ((1 << 128) // int(d)) >> 64] for d in mods], np.uint64)


def sr_tables(I, O, t):
    """ScaleAndRound tables, input moduli I, output moduli O: X_s = t * prod(O) * [(prod(I)prod(O)/s)^-1]_s;
    tab[j][i] = floor(X_{s_i}/s_i) mod o_j, tab[j][nI] = floor(X_{o_j}/o_j) mod o_j, frac[i] = float(X_{s_i} mod s_i)/float(s_i)"""
    I, O = [int(v) for v in I], [int(v) for v in O]
    B, M = prod(I) * prod(O), prod(O)
    X = lambda s: t * M * pow((B // s) % s, -1, s)
    tab = np.array([[(X(s) // s) % o for s in I] + [(X(o) // o) % o] for o in O], np.uint64).reshape(len(O), len(I) + 1)
    frac = np.array([float(X(s) % s) / float(s) for s in I], np.float64)
    return tab, frac


def tables(q, r, t, technique):
    """{(name, level): flat array} in the layout of fhe_hps_table (doubles as float64 arrays)"""
    q, r = [int(v) for v in q], [int(v) for v in r]
    nQ, nR = len(q), len(r)
    hps = technique == HPS
    T = {}
    T["qInv", 0] = np.array([1.0 / float(v) for v in q], np.float64)
    T["rInv", 0] = np.array([1.0 / float(v) for v in r], np.float64)
    T["qInvModr", 0] = np.array([[pow(s % d, -1, d) for d in r] for s in q], np.uint64).ravel()
    tab, frac = sr_tables(q, r, t)
    T["tRSHatInvModsDivsModr", 0], T["tRSHatInvModsDivsFrac", 0] = tab.ravel(), frac
    Q = prod(q)
    for l in range(nQ):
        L = l + 1
        Ql, rest = q[:L], q[L:]
        tab, frac = sr_tables(rest, Ql, 1)
        T["QlQHatInvModqDivqModq", l], T["QlQHatInvModqDivqFrac", l] = tab.ravel(), frac
        T["QlHatModq", l] = np.array([prod(rest) % s for s in Ql], np.uint64)
        if hps and l != nQ - 1:
            continue
        lev = 0 if hps else l
        Rl = r if hps else r[:L]
        for (S, D, names) in ((Ql, Rl, ("QlHatInvModq", "QlHatModr", "alphaQlModr")), (Rl, Ql, ("RlHatInvModr", "RlHatModq", "alphaRlModq"))):
            hatInv, _, hatMod, alpha, _, _ = libs.crt_tables(S, D)
            T[names[0], lev], T[names[1], lev], T[names[2], lev] = hatInv, hatMod.ravel(), alpha.ravel()
        if hps:
            continue
        tab, frac = sr_tables(Rl, Ql, t)
        T["tQlSlHatInvModsDivsModq", l], T["tQlSlHatInvModsDivsFrac", l] = tab.ravel(), frac
        R, QL = prod(Rl), prod(Ql)
        T["negRlQHatInvModq", l] = np.array([s - (R * pow((Q // s) % s, -1, s)) % s for s in q], np.uint64)
        T["negRlQlHatInvModq", l] = np.array([s - (R * pow((QL // s) % s, -1, s)) % s for s in Ql], np.uint64)
    return {k: v for k, v in T.items() if v.size}  # (the top level's Q -> Q_l fractions are an empty vector: no table)


def table_of(plan, name, level):
    """the plan's table with the dtype of tables()'s entry"""
    v = plan.table(name, level)
    if v is None:
        return None
    return v.view(np.float64) if name in ("qInv", "rInv") or name.endswith("Frac") else v


class Composer:
    """EvalMult of the HPS family on HOST towers, one ciphertext pair at a time, from the oracle's members"""

    def __init__(self, o, N, q, psiQ, r, psiR, t, technique):
        self.o, self.N, self.t, self.technique = o, N, int(t), technique
        self.q, self.r = np.ascontiguousarray(q, np.uint64), np.ascontiguousarray(r, np.uint64)
        self.nQ, self.nR = len(q), len(r)
        allq = np.concatenate([self.q, self.r])
        allpsi = np.concatenate([np.asarray(psiQ, np.uint64), np.asarray(psiR, np.uint64)])
        self.octx = o.orc_ctx_create(N, len(allq), allq, allpsi)

    def close(self):
        if self.octx:
            self.o.orc_ctx_destroy(self.octx)
            self.octx = None

    def ntt(self, x, idx, inverse):
        x = np.ascontiguousarray(x, np.uint64).copy()
        idx = np.ascontiguousarray(idx, np.uint32)
        f = self.o.orc_ntt_inv_tower if inverse else self.o.orc_ntt_fwd_tower
        f(self.octx, x, idx.ctypes.data, len(idx), 1, 1)
        return x

    def switch_exact(self, x, S, D):
        hatInv, hatPre, hatMod, alpha, inv, mu = libs.crt_tables(S, D)
        out = np.zeros((len(D), self.N), np.uint64)
        self.o.orc_switch_crt_basis(np.ascontiguousarray(x), len(S), self.N, np.ascontiguousarray(S), hatInv, hatPre,
                                    np.ascontiguousarray(hatMod.T), alpha, len(D), np.ascontiguousarray(D), mu, inv, out)
        return out

    def scale_round(self, x, I, O, t, output_first):
        tab, frac = sr_tables(I, O, t)
        O = np.ascontiguousarray(O, np.uint64)
        out = np.zeros((len(O), self.N), np.uint64)
        self.o.orc_scale_and_round(np.ascontiguousarray(x), len(I), len(O), self.N, 1 if output_first else 0, tab, frac, O, mu128(O), out)
        return out

    def eval_mult(self, A, B, size_ql=None):
        """A, B: [2][nQ][N] EVALUATION -> [3][nQ][N] COEFFICIENT"""
        o, N, q, r, nQ, t = self.o, self.N, self.q, self.r, self.nQ, self.t
        hps = self.technique == HPS
        L = nQ if size_ql is None else size_ql
        assert 1 <= L <= nQ and (L == nQ or self.technique == HPSPOVERQLEVELED)
        Ql, Rl = q[:L].copy(), (r if hps else r[:L]).copy()
        Lr = len(Rl)
        qidx = np.arange(nQ, dtype=np.uint32)
        idx = np.concatenate([np.arange(L, dtype=np.uint32), np.arange(nQ, nQ + Lr, dtype=np.uint32)])
        mods = np.concatenate([Ql, Rl])

        def expand(coef):  # ExpandCRTBasis Q_l -> Q_lR_l, result EVALUATION
            return self.ntt(np.concatenate([coef, self.switch_exact(coef, Ql, Rl)]), idx, False)

        def operand_a(x):
            coef = self.ntt(x, qidx, True)
            if L < nQ:
                coef = self.scale_round(coef, q[L:], Ql, 1, True)
            return expand(coef)

        def operand_b(x):
            if hps:
                return operand_a(x)
            coef = self.ntt(x, qidx, True)
            m, mpre, qinvp = libs.p_over_q_tables(q, Rl)  # at the top level Q_l = Q: mNegRlQlHatInvModq = mNegRlQHatInvModq
            hatInv2, hatPre2, hatMod2, alpha2, rInv, muQl = libs.crt_tables(Rl, Ql)
            out = np.zeros((L + Lr, N), np.uint64)
            o.orc_fast_expand_crt_basis_p_over_q(coef, nQ, N, q, m, mpre, qinvp, Lr, Rl, mu128(Rl), hatInv2, hatPre2,
                                                 np.ascontiguousarray(hatMod2.T), alpha2, L, Ql, muQl, rInv, out)
            return self.ntt(out, idx, False)

        a = [operand_a(A[0]), operand_a(A[1])]
        b = [operand_b(B[0]), operand_b(B[1])]

        def mul(x, y):
            z = np.empty_like(x)
            for i, m in enumerate(mods):
                o.orc_vec_mul(z[i], np.ascontiguousarray(x[i]), np.ascontiguousarray(y[i]), N, int(m))
            return z

        def add(x, y):
            z = np.empty_like(x)
            for i, m in enumerate(mods):
                o.orc_vec_add(z[i], np.ascontiguousarray(x[i]), np.ascontiguousarray(y[i]), N, int(m))
            return z

        prods = [mul(a[0], b[0]), add(mul(a[0], b[1]), mul(a[1], b[0])), mul(a[1], b[1])]
        D = np.zeros((3, nQ, N), np.uint64)
        for k, p in enumerate(prods):
            p = self.ntt(p, idx, True)
            if hps:
                D[k] = self.switch_exact(self.scale_round(p, q, Rl, t, False), Rl, q)
                continue
            y = self.scale_round(p, Rl, Ql, t, True)
            if L < nQ:
                hat = np.array([prod(q[L:]) % int(s) for s in Ql], np.uint64)
                o.orc_expand_crt_basis_ql_hat(y, L, N, q, hat, nQ, D[k])
            else:
                D[k] = y
        return D


def chain(o, logN, bits, n):
    """the reference's BFV modulus chain: q_0 = LastPrime(bits, 2N), q_i = PreviousPrime(q_{i-1}, 2N), with the minimum roots"""
    M = 2 << logN
    q = [o.orc_last_prime(bits, M)]
    while len(q) < n:
        q.append(o.orc_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    return q, np.array([o.orc_root_of_unity(M, int(v)) for v in q], np.uint64)
