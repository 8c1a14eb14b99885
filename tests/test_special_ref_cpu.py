"""CPU self-tests of tests/special_ref.py: the reference agrees with torch's float64 functions, and
the comparator rejects the defects it exists to catch (planted here in numpy fp32)."""
import numpy as np
import pytest
import torch

from tests import special_ref as S

F32 = np.float32
P = S.PROBES


def _f32(fn, *a):
    with np.errstate(all="ignore"):
        return np.asarray(fn(*a)).astype(F32)


def test_probe_vectors():
    assert P.dtype == F32 and 150 <= P.size <= 350
    bits = set(P.view(np.uint32).tolist())
    for v in (0.0, -0.0, S.DENORM_MIN, -S.DENORM_MAX, S.FLT_MIN, -S.FLT_MAX, np.inf, -np.inf, 1.0, 9.02, -17.4):
        assert np.array([v], F32).view(np.uint32)[0] in bits, v
    assert 0x7FC00000 in bits and np.isnan(P).sum() == 1
    # the expf edges sit between their fp32 neighbours
    with np.errstate(over="ignore"):
        e64, e5 = np.exp(P.astype(np.float64)), np.exp((F32(0.2) * P).astype(np.float64))
    assert (np.isinf(_f32(lambda: e64)) & np.isfinite(P)).any()      # overflow reached by a finite probe
    assert ((e64 < 2.0 ** -150) & (e64 > 0)).any() and ((e64 >= 2.0 ** -149) & (e64 < S.FLT_MIN)).any()
    assert ((e5 < S.FLT_MIN) & (e5 > 2.0 ** -149) & (P < 0)).any()  # 0.2f * v reaches the denormal range
    pb = S.PROBES_BF16
    assert np.array_equal(S.bf16_round(pb).view(np.uint32), pb.view(np.uint32))   # representable in bf16
    assert (pb.view(np.uint32) & 0xFFFF == 0).all()
    assert S.bits_same(pb, torch.from_numpy(pb.copy()).to(torch.bfloat16).float().numpy()).all()
    assert len(set(pb.view(np.uint32).tolist())) == pb.size
    bp = S.bin_probes()
    assert bp.size == 24 and all(b in bits for b in bp.view(np.uint32).tolist())
    assert S.dense().size == P.size + 2 * 4096


def test_bf16_round_is_torchs():
    v = np.concatenate([S.dense(512), P])
    want = torch.from_numpy(v.copy()).to(torch.bfloat16).float().numpy()
    got = S.bf16_round(v)
    assert S.bits_same(got, want).all()


@pytest.mark.parametrize("kind,fn,rtol", [
    ("RELU", torch.relu, 0.0),
    ("ELU", torch.nn.functional.elu, 1e-13),
    # torch multiplies by the double 0.2; the kernels (and sf_ref) by 0.2f, 1.5e-8 away
    ("LEAKY_RELU", lambda t: torch.nn.functional.leaky_relu(t, 0.2), 1e-7),
    ("SIGMOID", torch.sigmoid, 1e-13),
    ("TANH", torch.tanh, 1e-13),
    ("RECIP", torch.reciprocal, 0.0),
    ("EXP", torch.exp, 1e-13),
])
def test_sf_ref_agrees_with_torch_float64(kind, fn, rtol):
    want = fn(torch.from_numpy(P.astype(np.float64))).numpy()
    got = S.sf_ref(kind, P)
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert np.array_equal(np.sign(got[~fin & ~np.isnan(want)]), np.sign(want[~fin & ~np.isnan(want)]))
    atol = 2.0 ** -149 if kind == "LEAKY_RELU" else 0.0   # the staged fp32 product underflows as the kernel's does
    assert np.all(np.abs(got[fin] - want[fin]) <= rtol * np.abs(want[fin]) + atol)
    if kind in ("RECIP", "TANH"):  # the zeros whose sign IEEE fixes
        z = S.zero_sign_fixed(kind, P)
        assert z.sum() == 2 and np.array_equal(np.signbit(got[z]), np.signbit(want[z]))


def test_sf_ref_staging():
    """exp(leaky(v)) is taken of the fp32 product 0.2f * v, not of the fp64 one."""
    v = np.array([-400.0, -515.0, 3.0], F32)
    got = S.sf_ref("EXP_LEAKY_RELU", v)
    assert np.array_equal(got[:2], np.exp((F32(0.2) * v[:2]).astype(np.float64))) and got[2] == np.exp(3.0)
    v = -np.linspace(300, 500, 201).astype(F32)
    unstaged = np.exp(0.2 * v.astype(np.float64))
    rel = np.abs(S.sf_ref("EXP_LEAKY_RELU", v) - unstaged) / unstaged
    assert rel.max() > 2e-6                                     # tens of ulp of input rounding kept out of the bound
    assert np.isnan(S.sf_ref("EXP_LEAKY_RELU", np.array([np.nan], F32))[0])


def test_sf_stated_is_sf_ref_but_for_the_sigmoid_tail():
    v = S.dense()
    for kind in S.SFS:
        a, b = S.sf_stated(kind, v), S.sf_ref(kind, v)
        diff = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        if kind != "SIGMOID":
            assert not diff.any()
            continue
        assert diff.any() and (v[diff] <= S.SIGMOID_FLUSH_FROM).all() and (a[diff] == 0).all()
        assert (b[diff] < 2.9e-39).all()                       # the flushed values are denormals
        with np.errstate(over="ignore"):                        # exactly where fp32 expf(-v) overflows
            over = np.exp(-v.astype(np.float64)) > float(S.FLT_MAX) * (1 + 2.0 ** -25)
        assert np.array_equal(over & (b > 0), diff)
    t = S.SIGMOID_FLUSH_FROM
    assert np.exp(-np.float64(t)) > float(S.FLT_MAX) > np.exp(-np.float64(np.nextafter(t, F32(0))))


def test_ulp_diff_and_same():
    x = np.array([1.0, 1e-3, 3e38, S.FLT_MIN, 2.0 ** -140, 0.0], F32)
    up = np.nextafter(x, F32(np.inf))
    assert np.allclose(S.ulp_diff(up, x.astype(np.float64)), 1.0)
    assert S.ulp_diff(np.array([0.0], F32), np.array([2.0 ** -130]))[0] == 2.0 ** 19   # a flushed denormal: 2^-149 units
    assert S.ulp_diff(np.array([np.inf], F32), np.array([float(S.FLT_MAX)]))[0] == 1.0
    assert S.same(x, x.astype(np.float64)).all() and not S.same(up, x.astype(np.float64)).any()
    assert S.same(up, x.astype(np.float64), ulps=1).all()
    nan, inf, z = F32(np.nan), F32(np.inf), F32(0)
    assert S.same(np.array([nan], F32), np.array([np.nan]))[0]
    assert S.same(np.array([0xFFC00001], np.uint32).view(F32), np.array([np.nan]))[0]      # any payload
    assert not S.same(np.array([z], F32), np.array([np.nan]), ulps=1e30)[0]
    assert not S.same(np.array([nan], F32), np.array([0.0]), ulps=1e30)[0]
    assert not S.same(np.array([-inf], F32), np.array([np.inf]), ulps=1e30)[0]
    assert not S.same(np.array([S.FLT_MAX], F32), np.array([np.inf]), ulps=1e30)[0]
    assert S.same(np.array([-z], F32), np.array([0.0]))[0]
    assert not S.same(np.array([-z], F32), np.array([0.0]), zero_sign=True)[0]
    assert S.same(np.array([-z, z], F32), np.array([0.0, 0.0]), zero_sign=np.array([False, True])).all()
    assert S.bits_same(np.array([nan, z], F32), np.array([0xFFC00001, 0], np.uint32).view(F32)).all()
    assert not S.bits_same(np.array([z], F32), np.array([-z], F32))[0]


@pytest.mark.parametrize("kind", S.SFS)
def test_correctly_rounded_sf_passes(kind):
    """The positive control: sf_ref rounded to fp32 is accepted at 0 ulp (1 for the double rounding
    of a staged result), with the fixed zero signs."""
    for v in (P, S.PROBES_BF16):
        got = _f32(S.sf_ref, kind, v)
        ok = S.same(got, S.sf_ref(kind, v), ulps=0.5, zero_sign=S.zero_sign_fixed(kind, v))
        assert ok.all(), S.describe(ok, v, got, S.sf_ref(kind, v))


def _planted_relu(v):
    return np.where(v > 0, v, F32(0))                       # the kernel before this suite: NaN -> 0


def _planted_sigmoid(v):
    e = np.exp(v)
    return e / (F32(1) + e)                                 # inf / inf from v = 88.8 up


def _planted_tanh(v):
    e = np.exp(F32(2) * v)
    return (e - F32(1)) / (e + F32(1))                      # cancels near 0, inf / inf from 44.4 up


def _planted_elu(v):
    return np.where(v > 0, v, np.exp(v) - F32(1))           # cancels near 0


@pytest.mark.parametrize("kind,planted", [("RELU", _planted_relu), ("SIGMOID", _planted_sigmoid),
                                          ("TANH", _planted_tanh), ("ELU", _planted_elu)])
def test_same_rejects_planted_sf(kind, planted):
    got = _f32(planted, P)
    ok = S.same(got, S.sf_ref(kind, P), ulps=S.SF_ULPS[kind], zero_sign=S.zero_sign_fixed(kind, P))
    assert not ok.all()
    if kind == "RELU":  # exactly the NaN probe
        assert np.array_equal(~ok, np.isnan(P))


@pytest.mark.parametrize("kind", [k for k in S.SFS if k != "RELU"])   # RELU is idempotent: that is the gap
def test_same_rejects_sf_applied_twice(kind):
    once = _f32(S.sf_ref, kind, P)
    twice = _f32(S.sf_ref, kind, once)
    ok = S.same(twice, S.sf_ref(kind, P), ulps=S.SF_ULPS[kind], zero_sign=S.zero_sign_fixed(kind, P))
    assert (~ok).sum() > P.size // 4
    assert S.same(_f32(S.sf_ref, "RELU", _f32(S.sf_ref, "RELU", P)), S.sf_ref("RELU", P)).all()


def test_same_rejects_division_through_a_reciprocal():
    b = S.bin_probes()
    a2, b2 = np.repeat(b, b.size), np.tile(b, b.size)
    want = S.bin_ref("DIV", a2, b2)
    assert S.same(want, want, zero_sign=True).all()
    with np.errstate(all="ignore"):
        got = (a2 * (F32(1) / b2)).astype(F32)
    assert not S.same(got, want, zero_sign=True).all()


def test_bin_ref_is_ieee():
    """Spot values of the IEEE table the GPU must reproduce bit for bit."""
    inf, nan = F32(np.inf), F32(np.nan)
    r = S.bin_ref
    one = lambda k, a, b: r(k, np.array([a], F32), np.array([b], F32))[0]
    assert np.isnan(one("SUB", inf, inf)) and np.isnan(one("MUL", 0.0, inf)) and np.isnan(one("DIV", 0.0, 0.0))
    assert np.isnan(one("DIV", inf, inf)) and np.isnan(one("ADD", nan, 1.0))
    assert one("DIV", 1.0, -0.0) == -inf and one("DIV", -1.0, inf) == 0 and np.signbit(one("DIV", -1.0, inf))
    assert one("MUL", S.FLT_MIN, 0.5) == F32(2.0 ** -127)              # denormals kept
    assert one("ADD", S.DENORM_MIN, S.DENORM_MIN) == F32(2.0 ** -148)
    assert one("DIV", S.FLT_MIN, 2.0) == F32(2.0 ** -127)
    assert one("ADD", S.FLT_MAX, S.FLT_MAX) == inf
