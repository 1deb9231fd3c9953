#!/usr/bin/env python3
"""BFV EvalMult of the HPS family at config 5's shape (N = 2^15, 60-bit limbs, 7 Q limbs, batch 64), on one GPU:

  (a) the composite fhe_bfv_eval_mult_hps (register-resident conversion kernels where the bases fit),
  (b) the same product issued member by member through the entry points that take the caller's tables (fhe_expand_crt_basis,
      fhe_fast_expand_crt_basis_p_over_q, fhe_scale_and_round, fhe_switch_basis_exact, fhe_expand_crt_basis_ql_hat, fhe_tensor, NTTs),
  (c) for context, fhe_bfv_eval_mult_behz.

Every variant is recorded once into a graph and replayed; (a) and (b) alternate in one process after warm-up, `--repeats` times,
and the table reports median and spread.  The outputs of (a) and (b) must be identical (fhe_checksum of all three elements).
A tool, not a test: it fails without a GPU.   python tools/bfv_hps_bench.py [--out profiles/FILE.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openfhe_amd import fhe_hip as fh  # noqa: E402

u32p, u64p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p
f64p = C.POINTER(C.c_double)


def idx(v):
    a = np.ascontiguousarray(np.asarray(v, np.uint32))
    return a, a.ctypes.data_as(u32p)


class Members:
    """the member sequence of LeveledSHEBFVRNS::EvalMult with caller tables (read back from the plan: the same values)"""

    def __init__(self, lib, ctx, plan, numQ, numR, tech, size_ql, batch):
        self.lib, self.ctx, self.L, self.tech, self.batch = lib, ctx, lib.L, tech, batch
        L_ = self.L
        self.nQ, self.Lq = numQ, size_ql
        self.Lr = numR if tech == fh.HPS else size_ql
        lev = 0 if tech == fh.HPS else size_ql - 1
        self.keep = []
        self.qidx, self.qidx_p = idx(np.arange(numQ))
        qi, qi_p = idx(np.arange(size_ql))
        ri, ri_p = idx(np.arange(numQ, numQ + self.Lr))
        self.all, self.all_p = idx(np.concatenate([qi, ri]))
        self.keep += [qi, ri]
        self.tot = size_ql + self.Lr

        def conv(s, sp, ns, d, dp, nd, hat_inv=None, hat_mod=None):
            h = vp()
            if hat_inv is None:
                lib.check(L_.fhe_conv_create(ctx.h, sp, ns, dp, nd, C.byref(h)))
            else:
                hat_inv, hat_mod = np.ascontiguousarray(hat_inv), np.ascontiguousarray(hat_mod)
                lib.check(L_.fhe_conv_create_custom(ctx.h, sp, ns, dp, nd, hat_inv.ctypes.data_as(u64p), hat_mod.ctypes.data_as(u64p),
                                                    None, None, C.byref(h)))
            return h

        def sr(name, size_i, out_p, size_o):
            tab = plan.table(name + "Mod" + ("r" if name.startswith("tRS") else "q"), lev)
            frac = plan.table(name + "Frac", lev).view(np.float64)
            h = vp()
            lib.check(L_.fhe_sr_plan_create(ctx.h, size_i, out_p, size_o, tab.ctypes.data_as(u64p), frac.ctypes.data_as(f64p), C.byref(h)))
            return h

        self.q_to_r = conv(qi, qi_p, size_ql, ri, ri_p, self.Lr)
        self.r_to_q = conv(ri, ri_p, self.Lr, qi, qi_p, size_ql)
        if tech == fh.HPS:
            self.tail = sr("tRSHatInvModsDivs", numQ, ri_p, self.Lr)
        else:
            self.tail = sr("tQlSlHatInvModsDivs", self.Lr, qi_p, size_ql)
            neg = plan.table("negRlQHatInvModq", lev)
            inv = plan.table("qInvModr", 0).reshape(numQ, numR)[:, :self.Lr]
            self.p_over_q = conv(self.qidx, self.qidx_p, numQ, ri, ri_p, self.Lr, neg, inv)
            if size_ql < numQ:
                self.drop = sr("QlQHatInvModqDivq", numQ - size_ql, qi_p, size_ql)
                self.hat = plan.table("QlHatModq", lev)
        N = ctx.N
        rows = lambda n: batch * n * N * 8
        self.e = [ctx.malloc(rows(self.tot)) for _ in range(4)]
        self.p = [ctx.malloc(rows(self.tot)) for _ in range(3)]
        self.coef, self.tmp = ctx.malloc(rows(numQ)), ctx.malloc(rows(max(numQ, numR)))
        self.coef_bytes = rows(numQ)

    def run(self, ins, outs, st):
        lib, L_, c, B = self.lib, self.L, self.ctx.h, self.batch
        ck = lib.check
        hps, dropped = self.tech == fh.HPS, self.Lq < self.nQ
        for k in range(4):
            if hps or (k < 2 and not dropped):
                ck(L_.fhe_expand_crt_basis(self.q_to_r, ins[k], 1, self.e[k], 1, 0, B, self.coef, self.coef_bytes, st))
                continue
            ck(L_.fhe_ntt_inv_oop(c, ins[k], self.coef, self.qidx_p, self.nQ, B, st))
            if k < 2:
                ck(L_.fhe_scale_and_round(self.drop, self.coef, 1, self.tmp, B, st))
                ck(L_.fhe_expand_crt_basis(self.q_to_r, self.tmp, 0, self.e[k], 1, 0, B, None, 0, st))
            else:
                ck(L_.fhe_fast_expand_crt_basis_p_over_q(self.p_over_q, self.r_to_q, self.coef, self.e[k], B, st))
                ck(L_.fhe_ntt_fwd(c, self.e[k], self.all_p, self.tot, B, st))
        ck(L_.fhe_tensor(c, self.e[0], self.e[1], self.e[2], self.e[3], self.p[0], self.p[1], self.p[2], self.all_p, self.tot, B, st))
        for k in range(3):
            ck(L_.fhe_ntt_inv(c, self.p[k], self.all_p, self.tot, B, st))
            if hps:
                ck(L_.fhe_scale_and_round(self.tail, self.p[k], 0, self.tmp, B, st))
                ck(L_.fhe_switch_basis_exact(self.r_to_q, self.tmp, self.Lr, 0, outs[k], self.nQ, 0, B, st))
            elif not dropped:
                ck(L_.fhe_scale_and_round(self.tail, self.p[k], 1, outs[k], B, st))
            else:
                ck(L_.fhe_scale_and_round(self.tail, self.p[k], 1, self.tmp, B, st))
                ck(L_.fhe_expand_crt_basis_ql_hat(c, self.tmp, self.Lq, self.hat.ctypes.data_as(u64p), self.qidx_p, self.nQ, B, outs[k], st))


def capture(lib, ctx, st, call):
    call()
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    g = vp()
    lib.check(lib.L.fhe_graph_begin(ctx.h, st))
    call()
    lib.check(lib.L.fhe_graph_end(ctx.h, st, C.byref(g)))
    return g


def timed(lib, ctx, st, g, n):
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    t0 = time.perf_counter()
    for _ in range(n):
        lib.check(lib.L.fhe_graph_launch(ctx.h, g, st))
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logN", type=int, default=15)
    ap.add_argument("--limbs", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100, help="graph launches per timed repeat")
    ap.add_argument("--out", default=None, help="write the table (markdown) to this file")
    a = ap.parse_args()
    assert a.repeats >= 5
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bfv_hps_bench: needs the HIP build and a GPU")
    logN, numQ, B, t = a.logN, a.limbs, a.batch, 65537
    M = 2 << logN
    q = [lib.L.fhe_param_last_prime(60, M)]
    while len(q) < numQ:
        q.append(lib.L.fhe_param_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    psiQ = np.array([lib.L.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)
    rng = np.random.default_rng(5)
    rows = []
    cases = [("HPS", fh.HPS, numQ), ("HPSPOVERQ", fh.HPSPOVERQ, numQ), ("HPSPOVERQLEVELED", fh.HPSPOVERQLEVELED, numQ),
             ("HPSPOVERQLEVELED, one level dropped", fh.HPSPOVERQLEVELED, numQ - 1)]
    for name, tech, size_ql in cases:
        r, psiR = lib.hps_r(logN, q, tech)
        ctx = fh.Context(lib, logN, np.concatenate([q, r]), np.concatenate([psiQ, psiR]))
        plan = fh.Hps(ctx, np.arange(numQ), np.arange(numQ, numQ + len(r)), t, tech)
        N = ctx.N
        host = np.empty((B, numQ, N), np.uint64)
        ins = []
        for _ in range(4):
            for i, qi in enumerate(q):
                host[:, i, :] = rng.integers(0, int(qi), size=(B, N), dtype=np.uint64)
            ins.append(ctx.tower(host, limb_idx=np.arange(numQ)))
        da = [ins[0].like() for _ in range(3)]
        db = [ins[0].like() for _ in range(3)]
        wsb = plan.workspace_bytes(size_ql, B)
        ws = ctx.malloc(wsb)
        st = vp()
        lib.check(lib.L.fhe_stream_create(ctx.h, C.byref(st)))
        mem = Members(lib, ctx, plan, numQ, len(r), tech, size_ql, B)
        ip, ap_, bp = [x.ptr for x in ins], [x.ptr for x in da], [x.ptr for x in db]
        call_a = lambda: lib.check(lib.L.fhe_bfv_eval_mult_hps(plan.h, ip[0], ip[1], ip[2], ip[3], ap_[0], ap_[1], ap_[2], size_ql, 0, B,
                                                               ws, wsb, st))
        call_b = lambda: mem.run(ip, bp, st)
        ga, gb = capture(lib, ctx, st, call_a), capture(lib, ctx, st, call_b)
        for k in range(3):
            sa, sb = ctx.checksum(da[k]), ctx.checksum(db[k])
            assert np.array_equal(sa, sb), f"{name}: composite and member sequence differ in element {k}"
        for g in (ga, gb):  # warm-up
            timed(lib, ctx, st, g, a.inner)
        ta, tb = [], []
        for _ in range(a.repeats):
            ta.append(timed(lib, ctx, st, ga, a.inner))
            tb.append(timed(lib, ctx, st, gb, a.inner))
        rows.append({"technique": name, "sizeQl": size_ql, "composite_ms": ta, "members_ms": tb})
        lib.L.fhe_graph_destroy(ga)
        lib.L.fhe_graph_destroy(gb)
        lib.check(lib.L.fhe_stream_destroy(ctx.h, st))
        plan.close()
        ctx.close()
    # (c) BEHZ for context
    bsk, psiB = lib.behz_bsk(logN, q, t)
    ctx = fh.Context(lib, logN, np.concatenate([q, bsk]), np.concatenate([psiQ, psiB]))
    behz = fh.Behz(ctx, np.arange(numQ), np.arange(numQ, numQ + len(bsk)), t)
    host = np.empty((B, numQ, ctx.N), np.uint64)
    ins = []
    for _ in range(4):
        for i, qi in enumerate(q):
            host[:, i, :] = rng.integers(0, int(qi), size=(B, ctx.N), dtype=np.uint64)
        ins.append(ctx.tower(host, limb_idx=np.arange(numQ)))
    d = [ins[0].like() for _ in range(3)]
    wsb = lib.L.fhe_bfv_eval_mult_behz_workspace_bytes(behz.h, B)
    ws = ctx.malloc(wsb)
    st = vp()
    lib.check(lib.L.fhe_stream_create(ctx.h, C.byref(st)))
    g = capture(lib, ctx, st, lambda: lib.check(lib.L.fhe_bfv_eval_mult_behz(behz.h, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr,
                                                                              d[0].ptr, d[1].ptr, d[2].ptr, 0, B, ws, wsb, st)))
    timed(lib, ctx, st, g, a.inner)
    tc = [timed(lib, ctx, st, g, a.inner) for _ in range(a.repeats)]
    lib.L.fhe_graph_destroy(g)
    lib.check(lib.L.fhe_stream_destroy(ctx.h, st))
    behz.close()
    ctx.close()

    med = lambda v: float(np.median(v))
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    lines = [f"BFV EvalMultNoRelin, N = 2^{logN}, {numQ} Q limbs of 60 bits, batch {B}; ms per batch, median (min .. max) of {a.repeats} "
             f"repeats of {a.inner} graph launches, composite and member sequence alternating; outputs identical (fhe_checksum)", "",
             "| technique | composite | member sequence | members / composite |", "|---|---|---|---|"]
    for r_ in rows:
        lines.append(f"| {r_['technique']} | {fmt(r_['composite_ms'])} | {fmt(r_['members_ms'])} | "
                     f"{med(r_['members_ms']) / med(r_['composite_ms']):.3f} |")
    lines.append(f"| BEHZ (fhe_bfv_eval_mult_behz) | {fmt(tc)} | | |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows, "behz_ms": tc}))


if __name__ == "__main__":
    main()
