"""fhe_rescale_multi_limbs_pair against words recorded from the reference itself: the rescale of a CKKS product under COMPOSITESCALINGMANUAL
(LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, compositeDegree), ckksrns-leveledshe.cpp:172-191) at ring dimension 64 for composite
degree 2 and 3, with the reference's own tables GetQlQlInvModqlDivqlModq / GetqlInvModq of every step
(tests/golden/ref_vectors_ckks_composite.npz, written by tests/golden/make_golden_ckks_composite.py).  Every word is compared."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_ckks_composite.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("degree", [2, 3])
def test_composite_rescale_is_the_references(backend, golden, degree):
    g = golden
    ring, d, sizeQ, sizeQl, after = (int(v) for v in g[f"meta_d{degree}"])
    assert d == degree and after == sizeQl - degree and sizeQl == sizeQ
    q, psi, x, y = g[f"q_d{degree}"], g[f"psi_d{degree}"], g[f"x_d{degree}"], g[f"y_d{degree}"]
    ta, tb = g[f"tabA_d{degree}"], g[f"tabB_d{degree}"]
    assert len(ta) == len(tb) == sum(sizeQl - 1 - k for k in range(degree))
    # the tables are the negated pair of the inverses: what lets the steps collapse on the larger rings
    off = 0
    for k in range(degree):
        ql = int(q[sizeQl - 1 - k])
        for i in range(sizeQl - 1 - k):
            qi = int(q[i])
            assert int(tb[off + i]) == pow(ql % qi, -1, qi) and int(ta[off + i]) == (qi - int(tb[off + i])) % qi
        off += sizeQl - 1 - k
    logN = ring.bit_length() - 1
    ctx = fh.Context(backend, logN, q, psi)
    x0, x1 = ctx.tower(np.ascontiguousarray(x[0:1])), ctx.tower(np.ascontiguousarray(x[1:2]))
    r0, r1 = fh.rescale_multi_pair(ctx, x0, x1, degree, ta, tb)
    assert np.array_equal(r0.to_host()[0], y[0]) and np.array_equal(r1.to_host()[0], y[1])
    # ... and the library's own tables over the leading limbs give the same words
    both = fh.rescale_multi(ctx, ctx.tower(np.ascontiguousarray(x)), degree).to_host()
    assert np.array_equal(both, y)
    ctx.close()
