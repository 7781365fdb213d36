"""GPU parity of ofhe_hip_ks_eval_mult / ofhe_hip_ks_relinearize / ofhe_hip_ks_rescale, bit for bit against the
restatement in tests/she_mult_ref.py (pinned on the CPU by tests/test_she_mult_oracle.py).

Shapes are (log_n, size_q, size_p, dnum, size_ql, batch), the smallest that reach each path of the new code:
  (4, 3, 1, 3, 3, 1), (11, 4, 2, 2, 3, 3)   k_small + k_sub_scale_add, full and lower level
  (12, 4, 2, 2, 4, 2)                        the block pass alone (k_block_add NR = 3), no column pass
  (13, 5, 2, 3, 5, 3), (14, 4, 1, 2, 3, 5)   column pass + block pass, batch % 4 != 0, the switch-loading
                                             column pass in the rescale
  (16, 4, 2, 2, 4, 3)                        the k_tcols split (k_block_add NR = 2, a ragged quad)
  (17, 3, 1, 3, 3, 1)                        the ModDown with its inverse column pass inside the conversion
The reference of a shape is computed once and shared by the tests that use it."""
import functools

import numpy as np
import pytest

import keyswitch as K
import oracle as O
import she_mult_ref as S
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay: a fixture)
from test_gpu_keyswitch import _generic_bases
from test_gpu_parity import dev, host, stream
from tier2_cases import _moduli, valid_splits

pytestmark = pytest.mark.gpu

SHAPES = {4: (4, 3, 1, 3, 3, 1), 11: (11, 4, 2, 2, 3, 3), 12: (12, 4, 2, 2, 4, 2), 13: (13, 5, 2, 3, 5, 3),
          14: (14, 4, 1, 2, 3, 5), 16: (16, 4, 2, 2, 4, 3), 17: (17, 3, 1, 3, 3, 1)}
SCHEMES = [(S.CKKS, 0), (S.BGV, 2), (S.BGV, 65537)]
SCHEME_IDS = ["ckks", "bgv-t2", "bgv-t65537"]


def _uniform(rng, batch, moduli, n):
    return np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in moduli]) for _ in range(batch)])


@functools.lru_cache(maxsize=None)
def bases(log_n, sq, sp, kind):
    """chain: the poly-benchmark chain; generic: moduli far from 2^60; mixed: the tier-2 key-switch draw from
    22 bits on (towers of 22 to 60 bits, special and generic forms, in one engine)."""
    if kind == "generic":
        return _generic_bases(log_n, sq, sp)
    if kind == "mixed":
        for seed in range(64):  # the first draw whose towers span 25 bits or more
            m, r, _ = _moduli(np.random.default_rng([91, log_n, seed]), log_n, sq + sp, 22)
            if max(m).bit_length() - min(m).bit_length() >= 25:
                break
        else:
            raise AssertionError("no mixed draw")
    else:
        m, r = O.moduli_chain(log_n, sq + sp)
    return m[:sq], r[:sq], m[sq:], r[sq:]


class Case:
    """Operands, keys and lazily computed references of one shape."""

    def __init__(self, shape, kind="chain", data="uniform", nelem=4):
        self.log_n, self.sq, self.sp, self.dnum, self.l, self.B = shape
        self.n = 1 << self.log_n
        self.q, self.rq, self.p, self.rp = bases(self.log_n, self.sq, self.sp, kind)
        self.kp = K.KeySwitchParams(self.n, self.q, self.rq, self.p, self.rp, self.dnum)
        rng = np.random.default_rng([self.log_n, self.l, self.B])
        ql, qp = self.q[:self.l], self.q + self.p
        if data == "uniform":
            self.cv = [_uniform(rng, self.B, ql, self.n) for _ in range(nelem)]
            self.keys = [(_uniform(rng, self.dnum, qp, self.n), _uniform(rng, self.dnum, qp, self.n))
                         for _ in range(2)]
        else:  # every word at q - 1, or at zero
            def fill(batch, mods):
                m = np.array(mods, np.uint64)[None, :, None]
                return np.broadcast_to(m - 1 if data == "max" else m * 0, (batch, len(mods), self.n)).copy()

            self.cv = [fill(self.B, ql) for _ in range(nelem)]
            self.keys = [(fill(self.dnum, qp), fill(self.dnum, qp)) for _ in range(2)]
        self._ref = {}

    def mult_ref(self, square, scheme, t, levels):
        """The restatement's EvalMult / EvalSquare + `levels` rescalings; the levels build on one another."""
        key = (square, scheme, t, levels)
        if key not in self._ref:
            c0, c1, d0, d1 = self.cv[:4]
            kb, ka = self.keys[0]
            if levels == 0:
                self._ref[key] = S.eval_mult(self.kp, c0, c1, None if square else d0, None if square else d1, kb, ka,
                                             scheme, t, 0)
            else:
                prev = self.mult_ref(square, scheme, t, levels - 1)
                self._ref[key] = tuple(S.rescale(self.kp, list(prev), scheme, t, 1))
        return self._ref[key]


@functools.lru_cache(maxsize=None)
def case(log_n, kind="chain", data="uniform"):
    return Case(SHAPES[log_n], kind, data)


def engine(H, ctx, c, options=None):
    return H.KeySwitch(ctx, c.log_n, c.q, c.rq, c.p, c.rp, c.dnum, options)


def run_mult(ks, c, square, scheme, t, levels, st=None, place=None):
    """ks.eval_mult / eval_square on fresh device copies; place: operand indices whose buffers take out0, out1."""
    import torch

    ops = [dev(x) for x in c.cv[:4]]
    kb, ka = dev(c.keys[0][0]), dev(c.keys[0][1])
    if place is None:
        o0 = torch.zeros((c.B, c.l - levels, c.n), dtype=torch.int64, device="cuda")
        o1 = torch.zeros_like(o0)
    else:
        o0, o1 = ops[place[0]], ops[place[1]]
    d0, d1 = (0, 0) if square else (ops[2].data_ptr(), ops[3].data_ptr())
    ks.eval_mult(c.l, ops[0].data_ptr(), ops[1].data_ptr(), d0, d1, kb.data_ptr(), ka.data_ptr(), o0.data_ptr(),
                 o1.data_ptr(), scheme, t, levels, c.B, st if st is not None else stream())
    words = c.B * (c.l - levels) * c.n
    return [host(o).reshape(-1)[:words].reshape(c.B, c.l - levels, c.n) for o in (o0, o1)]


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("scheme,t", SCHEMES, ids=SCHEME_IDS)
@pytest.mark.parametrize("square", [False, True], ids=["product", "square"])
@pytest.mark.parametrize("log_n", [12, 13])
def test_eval_mult_full_cross(hip, log_n, square, scheme, t):
    H, ctx = hip
    c = case(log_n)
    ks = engine(H, ctx, c)
    for levels in (0, 1, 2):
        assert same(run_mult(ks, c, square, scheme, t, levels), c.mult_ref(square, scheme, t, levels)), levels
    ks.close()


@pytest.mark.parametrize("scheme,t", [SCHEMES[0], SCHEMES[2]], ids=["ckks", "bgv-t65537"])
@pytest.mark.parametrize("log_n", [4, 11, 14, 16, 17])
def test_eval_mult_other_shapes(hip, log_n, scheme, t):
    H, ctx = hip
    c = case(log_n)
    ks = engine(H, ctx, c)
    for square in (False, True):
        assert same(run_mult(ks, c, square, scheme, t, 1), c.mult_ref(square, scheme, t, 1)), square
    ks.close()


@pytest.mark.parametrize("t", [0, 65537])
@pytest.mark.parametrize("log_n", [11, 13, 17])
def test_relinearize(hip, log_n, t):
    """nelem 3 and 4, out of place and onto c[0], c[1]."""
    import torch

    H, ctx = hip
    c = case(log_n)
    ks = engine(H, ctx, c)
    keys = [(dev(kb), dev(ka)) for kb, ka in c.keys]
    for nelem in (3, 4):
        want = S.relinearize(c.kp, c.cv[:nelem], c.keys[:nelem - 2], t)
        for in_place in (False, True):
            cv = [dev(x) for x in c.cv[:nelem]]
            o0, o1 = (cv[0], cv[1]) if in_place else (torch.zeros_like(cv[0]), torch.zeros_like(cv[0]))
            ks.relinearize(c.l, [x.data_ptr() for x in cv], [k[0].data_ptr() for k in keys[:nelem - 2]],
                           [k[1].data_ptr() for k in keys[:nelem - 2]], o0.data_ptr(), o1.data_ptr(), t, c.B,
                           stream())
            assert same([host(o0), host(o1)], want), (nelem, in_place)
            if not in_place:
                assert all(np.array_equal(host(x), w) for x, w in zip(cv, c.cv))  # inputs untouched
    ks.close()


RESCALE_SHAPES = {10: (10, 4, 1, 2, 4, 2), 12: (12, 4, 1, 2, 4, 2), 14: (14, 4, 1, 2, 4, 3), 16: (16, 4, 1, 2, 4, 3)}


@pytest.mark.parametrize("scheme,t", [SCHEMES[0], SCHEMES[2]], ids=["ckks", "bgv-t65537"])
@pytest.mark.parametrize("log_n", [10, 12, 14, 16])
def test_rescale(hip, log_n, scheme, t):
    """nelem 2 and 3, levels 1 to 3; the elements are separate buffers."""
    import torch

    H, ctx = hip
    c = Case(RESCALE_SHAPES[log_n], nelem=3)
    ks = engine(H, ctx, c)
    want = {0: list(c.cv)}
    for levels in (1, 2, 3):
        want[levels] = S.rescale(c.kp, want[levels - 1], scheme, t, 1)
        for nelem in (2, 3):
            xs = [dev(x) for x in c.cv[:nelem]]
            outs = [torch.zeros((c.B, c.l - levels, c.n), dtype=torch.int64, device="cuda") for _ in range(nelem)]
            ks.rescale(c.l, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], scheme, t, levels, c.B, stream())
            assert same([host(o) for o in outs], want[levels][:nelem]), (levels, nelem)
            assert all(np.array_equal(host(x), w) for x, w in zip(xs, c.cv))
    ks.close()


def _settings(log_n):
    """(id, moduli kind, KsOptions fields) of the moduli and option settings of one ring size."""
    out = [("mixed", "mixed", {}), ("generic_moduli", "chain", {"generic_moduli": 1})]
    out += [(s, "chain", {"split": s}) for s in valid_splits(log_n)]
    out += [("chunk", "chain", {"chunk": 2 if SHAPES[log_n][5] > 2 else 1}), ("single_stream", "chain", {"single_stream": 1}),
            ("separate_cols", "chain", {"separate_cols": 1}), ("separate_icol", "chain", {"separate_icol": 1})]
    return [(log_n,) + s for s in out]


@pytest.mark.parametrize("log_n,name,kind,fields", [s for n in (13, 16, 17) for s in _settings(n)],
                         ids=[f"{s[0]}-{s[1]}" for n in (13, 16, 17) for s in _settings(n)])
def test_moduli_and_options(hip, log_n, name, kind, fields):
    """One product with levels = 1 per setting; every setting computes the same words."""
    H, ctx = hip
    shape = SHAPES[log_n]
    if name == "chunk" and shape[5] < 2:   # a chunk smaller than the batch needs a batch of two
        shape = shape[:5] + (2,)
    c = case(log_n, kind) if shape == SHAPES[log_n] else Case(shape, kind)
    opt = H.KsOptions()
    for k, v in fields.items():
        if k == "split":
            opt.plan.split = getattr(H, v)
        elif k == "generic_moduli":
            opt.plan.generic_moduli = v
        else:
            setattr(opt, k, v)
    ks = engine(H, ctx, c, opt)
    assert same(run_mult(ks, c, False, S.CKKS, 0, 1), c.mult_ref(False, S.CKKS, 0, 1))
    ks.close()


@pytest.mark.parametrize("scheme,t", [SCHEMES[0], SCHEMES[2]], ids=["ckks", "bgv-t65537"])
@pytest.mark.parametrize("data", ["max", "zero"])
@pytest.mark.parametrize("log_n", [11, 12, 13])
def test_edge_data(hip, log_n, data, scheme, t):
    """Operands and keys at q - 1 everywhere (the largest values the lazy chain of the new epilogue meets), and
    at zero."""
    H, ctx = hip
    c = case(log_n, "chain", data)
    ks = engine(H, ctx, c)
    for square in (False, True):
        for levels in (0, 1):
            assert same(run_mult(ks, c, square, scheme, t, levels), c.mult_ref(square, scheme, t, levels))
    ks.close()


@pytest.mark.parametrize("log_n", [11, 13])
def test_on_the_callers_stream(hip, delay, log_n):  # noqa: F811
    """From a non-default stream behind queued work, waited on through that stream alone."""
    H, ctx = hip
    c = case(log_n)
    ks = engine(H, ctx, c)
    for square, levels in ((False, 1), (True, 0)):
        run = OnStream(delay)
        ops = [run.input(x) for x in c.cv[:4]]
        kb, ka = run.input(c.keys[0][0]), run.input(c.keys[0][1])
        o0, o1 = run.output(c.B, c.l - levels, c.n), run.output(c.B, c.l - levels, c.n)
        run.begin()
        d0, d1 = (0, 0) if square else (ops[2].data_ptr(), ops[3].data_ptr())
        ks.eval_mult(c.l, ops[0].data_ptr(), ops[1].data_ptr(), d0, d1, kb.data_ptr(), ka.data_ptr(), o0.data_ptr(),
                     o1.data_ptr(), S.CKKS, 0, levels, c.B, run.h)
        run.fetch(o0, o1)
        assert same(run.wait(), c.mult_ref(square, S.CKKS, 0, levels)), (square, levels)
    import torch

    torch.cuda.synchronize()
    ks.close()


@pytest.mark.parametrize("log_n", [11, 13])
def test_in_place_forms(hip, log_n):
    """Outputs placed on the operands' buffers give the same words."""
    H, ctx = hip
    c = case(log_n)
    ks = engine(H, ctx, c)
    for place in ((0, 1), (2, 3), (1, 0), (3, 0)):
        for levels in (0, 1):
            assert same(run_mult(ks, c, False, S.CKKS, 0, levels, place=place), c.mult_ref(False, S.CKKS, 0, levels))
    assert same(run_mult(ks, c, True, S.BGV, 65537, 1, place=(0, 1)), c.mult_ref(True, S.BGV, 65537, 1))
    ks.close()


def test_refusals_leave_the_outputs_unwritten(hip):
    import torch

    H, ctx = hip
    c = case(11)
    ks = engine(H, ctx, c)
    l, B, n = c.l, c.B, c.n
    SENT = 0x5A5A5A5A
    big = torch.full((8, B, l, n), SENT, dtype=torch.int64, device="cuda")   # operands, outputs and overlaps inside
    for i, x in enumerate(c.cv[:4]):
        big[i].copy_(dev(x))
    kb, ka = dev(c.keys[0][0]), dev(c.keys[0][1])
    before = host(big).copy()
    P = lambda i, off=0: big[i].data_ptr() + 8 * off  # noqa: E731

    def refused(fn, *a, msg=None, **kw):
        with pytest.raises(H.MathError) as e:
            fn(*a, **kw)
        if msg:
            assert msg in str(e.value), str(e.value)
        assert np.array_equal(host(big), before)

    def mult(o0, o1, c0=P(0), c1=P(1), d0=P(2), d1=P(3), b=kb.data_ptr(), a=ka.data_ptr(), scheme=S.CKKS, t=0,
             levels=1, size_ql=l):
        ks.eval_mult(size_ql, c0, c1, d0, d1, b, a, o0, o1, scheme, t, levels, B, stream())

    refused(mult, P(0, n), P(5))                 # partial overlap with an operand
    refused(mult, P(4), P(1, 2 * n))
    refused(mult, P(4), P(4, n))                 # out0 overlapping out1
    refused(mult, kb.data_ptr(), P(5))           # an output on a key
    refused(mult, P(4), P(5), size_ql=c.sq + 1)  # size_ql outside the engine
    refused(mult, P(4), P(5), levels=l)          # levels >= size_ql
    refused(mult, P(4), P(5), d1=0)              # exactly one of d0, d1 NULL
    refused(mult, P(4), P(5), t=3)               # t with CKKS
    refused(mult, P(4), P(5), scheme=S.BGV, t=c.q[1], msg="q[1]")   # t not invertible: the tower is named
    refused(mult, P(4), P(5), scheme=S.BGV, t=c.p[0], msg="p[0]")
    cv = [P(i) for i in range(4)]
    keys_b, keys_a = [kb.data_ptr()] * 2, [ka.data_ptr()] * 2
    relin = lambda o0, o1, nelem=4: ks.relinearize(l, cv[:nelem], keys_b[:nelem - 2], keys_a[:nelem - 2], o0, o1, 0,  # noqa: E731
                                                   B, stream())
    refused(relin, P(1), P(5))                   # out0 on c[1]
    refused(relin, P(4), P(0))                   # out1 on c[0]
    refused(relin, P(2), P(5))                   # an output on a switched element
    refused(relin, P(0, n), P(5))                # partial overlap
    refused(relin, P(4), P(5), nelem=2)          # nelem < 3
    resc = lambda x, o, levels=1, scheme=S.CKKS, t=0: ks.rescale(l, x, o, scheme, t, levels, B, stream())  # noqa: E731
    refused(resc, [P(0), P(1)], [P(0), P(5)])    # in place is not offered
    refused(resc, [P(0), P(1)], [P(4), P(4, n)])  # outputs overlapping each other
    refused(resc, [P(0), P(1)], [P(4), P(1, n)])
    refused(resc, [P(0)], [P(4)], levels=0)
    refused(resc, [P(0)], [P(4)], levels=l)
    refused(resc, [P(0)], [P(4)], scheme=S.BGV, t=c.q[0], msg="q[0]")
    # and the engine still computes
    assert same(run_mult(ks, c, False, S.CKKS, 0, 1), c.mult_ref(False, S.CKKS, 0, 1))
    ks.close()
