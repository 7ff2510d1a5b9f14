"""The three overlap predicates of the contact stage (include/md_geom.h: md_obb_obb, md_obb_circle, md_obb_quad -- one source for
the kernels and the oracle, so GPU == oracle says nothing about them) against the float64 reference of tests/contact_ref.py, which
uses no separating axes.  CPU only, through the oracle's exports."""
import numpy as np
import pytest

import contact_ref as cr
import oracle_binding as ob


def _obb_obb(cs):
    lib, a, b, n = ob.load(), cs.A.ctypes.data, cs.B.ctypes.data, cs.A.itemsize
    return np.array([lib.ref_obb_obb(a + i * n, b + i * n) for i in range(len(cs.A))], bool)


def _obb_circle(cs):
    lib, a, n = ob.load(), cs.A.ctypes.data, cs.A.itemsize
    bx, by, r = (cs.B[k].tolist() for k in ("cx", "cy", "hl"))
    return np.array([lib.ref_obb_circle(a + i * n, bx[i], by[i], r[i]) for i in range(len(cs.A))], bool)


def _obb_quad(cs):
    lib, a, n, q = ob.load(), cs.A.ctypes.data, cs.A.itemsize, cs.quads.ctypes.data
    return np.array([lib.ref_obb_quad(a + i * n, q + 32 * i) for i in range(len(cs.A))], bool)


SETS = {"obb_obb": (cr.pair_cases, _obb_obb, lambda cs: cr.obb_obb(cs.A, cs.B)),
        "obb_circle": (cr.circle_cases, _obb_circle, lambda cs: cr.obb_circle(cs.A, cs.B["cx"], cs.B["cy"], cs.B["hl"])),
        "obb_quad": (cr.quad_cases, _obb_quad, lambda cs: cr.obb_quad(cs.A, cs.quads))}
GENERATORS = {"obb_obb": {"random", "touching", "corner", "cross", "contains", "contained"},
              "obb_circle": {"random", "touching", "corner", "contains"},
              "obb_quad": {"random_line", "random_walk", "touching", "corner", "cross", "contains", "contained", "long_strip"}}


@pytest.mark.parametrize("name", sorted(SETS))
def test_predicate_equals_float64_where_decided(name):
    make, got_fn, want_fn = SETS[name]
    cs = make()
    assert cs.A.flags["C_CONTIGUOUS"] and (cs.quads is None or cs.quads.flags["C_CONTIGUOUS"])
    assert set(cs.gen) == GENERATORS[name] and len(cs.A) >= 6000
    assert np.abs(np.stack([cs.A["cx"], cs.A["cy"]])).max() < 2000.0
    want, decided = want_fn(cs)
    got = got_fn(cs)
    print(name, "cases", len(cs.A), "undecided", int((~decided).sum()), cr.summarise(cs, want, decided))
    # the inputs: nearly all decided, hits and misses both well represented, every near-touching case on the side it was built on
    assert (~decided).sum() <= cr.UNDECIDED_CAP * len(decided), (name, int((~decided).sum()), len(decided))
    nd = int(decided.sum())
    assert (want & decided).sum() >= 0.25 * nd and (~want & decided).sum() >= 0.25 * nd, (name, int((want & decided).sum()), nd)
    apart, into = cs.gap == 0.01, cs.gap == -0.01
    assert apart.sum() > 1000 and into.sum() > 1000
    assert decided[apart | into].all(), "a case built at +-0.01 m is undecided at EPS = %g" % cr.EPS
    assert not want[apart].any(), "%s: cases built 0.01 m apart that the reference calls hits: %s" % (name, np.nonzero(want & apart)[0][:5])
    assert want[into].all(), "%s: cases built 0.01 m into each other that the reference calls misses: %s" % (name, np.nonzero(~want & into)[0][:5])
    # the predicate
    bad = np.nonzero(decided & (got != want))[0]
    detail = [(int(i), str(cs.gen[i]), float(cs.gap[i]), bool(want[i]), cs.A[i].tolist(),
               (cs.B[i] if cs.B is not None else cs.quads[i]).tolist()) for i in bad[:3]]
    assert len(bad) == 0, "%s: float32 differs from float64 on %d decided cases; first (index, generator, gap, want, A, other): %s" % (
        name, len(bad), detail)


def test_reference_needs_no_orientation():
    """the reference gives the same answer for a quad listed clockwise (the predicate under test does not: it is for CCW quads)"""
    cs = cr.quad_cases(seed=5, n=200)
    want, _ = cr.obb_quad(cs.A, cs.quads)
    flipped = np.ascontiguousarray(cs.quads.reshape(-1, 4, 2)[:, ::-1].reshape(-1, 8))
    again, _ = cr.obb_quad(cs.A, flipped)
    assert (want == again).all()
