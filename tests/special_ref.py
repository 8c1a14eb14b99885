"""TEST-ONLY numpy reference for special values: the SFs, the binary ops and the comparator
(include/gta.h, "Special values of the SFs").

  PROBES / PROBES_BF16  fixed fp32 vectors: +-0, denormals, FLT_MIN, FLT_MAX, +-inf, NaN, the edges
                        of expf (overflow, underflow to denormal and to zero) with their fp32
                        neighbours, the same edges x 5 (what 0.2f * v reaches), the small-argument
                        and saturation points of tanhf / expm1f / the sigmoid, the RECIP edges, and 64
                        log-spaced magnitudes per sign over [1e-6, 1e2].  PROBES_BF16: their bf16
                        roundings (the exactly representable ones unchanged).
  sf_ref(kind, v32)     the fp64 value of an SF on fp32 inputs, STAGED as tests/softmax_shift_ref.py
                        stages scores: the argument handed to the transcendental is formed in fp32
                        exactly as csrc writes it (np.float32(0.2) * v for the leaky forms, -v exact),
                        everything after it is fp64.  Unstaged, exp(0.2 v) at v = -400 would show about
                        40 ulp of input rounding that is not the kernel's error.
  sf_stated(kind, v32)  sf_ref with the one deviation gta.h states (SIGMOID's flushed denormal tail):
                        what the GPU tests compare against
  bin_ref(kind, a, b)   numpy fp32 arithmetic: IEEE add, subtract, multiply and divide are correctly
                        rounded, libgta is built without fast-math and HIP's default fp32 divide is the
                        correctly rounded one, so the expected result is numpy's bits, denormals kept.
  ulp_diff(got32, want) distance in fp32 ulps of want (a denormal or zero result: units of 2^-149)
  same(got32, want, ...) the comparator: equal NaN-ness (any payload), equal infinities with sign,
                        zeros equal whatever their sign except where zero_sign says the function's IEEE
                        result fixes it (zero_sign_fixed: RECIP(+-inf) = +-0, TANH(+-0) = +-0;
                        RECIP(+-0) = +-inf is the infinity rule), otherwise at most `ulps` ulp_diff.
  bits_same(a, b)       bitwise equality of two fp32 arrays, NaNs equal by position (any payload)
"""
import numpy as np

F32 = np.float32
SFS = ("RELU", "EXP_LEAKY_RELU", "ELU", "EXP", "LEAKY_RELU", "SIGMOID", "TANH", "RECIP")
BINS = ("ADD", "SUB", "MUL", "DIV")

# The largest ulp_diff of gta_apply_node against sf_ref over dense() (PROBES plus 4,096 log-spaced
# magnitudes per sign over [1e-6, 1e2]), measured on the MI355X ("Special values"), plus one
# ulp: the margin for another rounding of the same math library on another build, and no more.
SF_ULPS_MEASURED = {"RELU": 0.0, "LEAKY_RELU": 0.0, "RECIP": 0.5, "EXP": 1.0, "EXP_LEAKY_RELU": 1.0,
                    "ELU": 0.821, "TANH": 0.892, "SIGMOID": 1.953}
SF_ULPS = {k: v + 1.0 for k, v in SF_ULPS_MEASURED.items()}

FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny           # 2^-126
DENORM_MIN = F32(2.0 ** -149)
DENORM_MAX = np.nextafter(FLT_MIN, F32(0))
QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]


def _with_neighbours(x):
    x = F32(x)
    return [np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))]


def _probes():
    p = []
    for m in (0.0, DENORM_MIN, DENORM_MAX, FLT_MIN, 1.0, FLT_MAX, np.inf):
        p += [F32(m), -F32(m)]
    p.append(QNAN)
    edges = [np.log(np.float64(FLT_MAX)), np.log(np.float64(FLT_MIN)), np.log(2.0 ** -149)]
    for e in edges:                      # expf overflows / goes denormal / goes to zero here
        p += _with_neighbours(e)
    for e in edges:                      # the negative side x 5: what 0.2f * v hands to expf
        p += _with_neighbours(-abs(e) * 5.0)
    for m in (2.0 ** -12, 1e-4,          # small-argument branches of tanhf and expm1f
              9.0, 9.02,                 # tanh saturation
              16.6, 17.4,                # 1 + e^-v rounds to 1
              2.0 ** -126, 2.0 ** -127, 2.0 ** -128, 2.0 ** 126, 2.0 ** 127):  # RECIP to / from denormal and inf
        p += [F32(m), -F32(m)]
    mags = np.logspace(-6, 2, 64).astype(F32)
    p += list(mags) + list(-mags)
    return np.array(p, F32)


def bf16_round(v32):
    """fp32 values rounded to bf16 (round to nearest even), as fp32; NaN stays NaN."""
    v32 = np.ascontiguousarray(v32, F32)
    u = v32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    out = r.view(F32).copy()
    out[np.isnan(v32)] = QNAN
    return out


def _unique_bits(v32):
    _, idx = np.unique(v32.view(np.uint32), return_index=True)
    return v32[np.sort(idx)]


PROBES = _probes()
PROBES_BF16 = _unique_bits(bf16_round(PROBES))
PROBES.setflags(write=False)
PROBES_BF16.setflags(write=False)


def dense(n_per_sign=4096, lo=1e-6, hi=1e2):
    """PROBES plus n log-spaced magnitudes per sign: the inputs the per-SF ulp bound is measured on."""
    mags = np.logspace(np.log10(lo), np.log10(hi), n_per_sign).astype(F32)
    return np.concatenate([PROBES, mags, -mags])


def sf_arg(kind, v32):
    """The fp32 value csrc's sf_apply hands to the transcendental (or, for LEAKY_RELU, returns)."""
    v32 = np.asarray(v32)
    assert v32.dtype == F32
    if kind in ("EXP_LEAKY_RELU", "LEAKY_RELU"):
        with np.errstate(all="ignore"):
            return np.where(v32 > 0, v32, F32(0.2) * v32).astype(F32)
    if kind == "SIGMOID":
        return -v32
    return v32


def sf_ref(kind, v32):
    """fp64 value of SF `kind` on the fp32 inputs v32, staged (see the module docstring)."""
    v32 = np.asarray(v32)
    assert v32.dtype == F32
    v = v32.astype(np.float64)
    t = sf_arg(kind, v32).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind in (None, "NONE"):
            return v
        if kind == "RELU":
            return np.maximum(v, 0.0)            # propagates NaN
        if kind == "EXP_LEAKY_RELU":
            return np.exp(t)
        if kind == "ELU":
            return np.where(v > 0, v, np.expm1(v))
        if kind == "EXP":
            return np.exp(v)
        if kind == "LEAKY_RELU":
            return t
        if kind == "SIGMOID":
            return 1.0 / (1.0 + np.exp(t))
        if kind == "TANH":
            return np.tanh(v)
        if kind == "RECIP":
            return 1.0 / v
    raise ValueError(kind)


# from here down expf(-v) overflows in fp32 (the fp32 nearest ln(FLT_MAX), just above it)
SIGMOID_FLUSH_FROM = F32(-88.72284)


def sf_stated(kind, v32):
    """sf_ref with the one deviation gta.h states: SIGMOID is +0 where expf(-v) overflows
    (v <= -88.7228), although the exact value is a denormal down to v = -103.97."""
    want = sf_ref(kind, v32)
    if kind == "SIGMOID":
        want = np.where(np.asarray(v32) <= SIGMOID_FLUSH_FROM, 0.0, want)
    return want


def bin_ref(kind, a32, b32):
    """fp32 result of a `kind` b: numpy's correctly rounded IEEE arithmetic."""
    a32, b32 = np.asarray(a32), np.asarray(b32)
    assert a32.dtype == F32 and b32.dtype == F32
    with np.errstate(all="ignore"):
        if kind == "ADD":
            return (a32 + b32).astype(F32)
        if kind == "SUB":
            return (a32 - b32).astype(F32)
        if kind == "MUL":
            return (a32 * b32).astype(F32)
        if kind == "DIV":
            return (a32 / b32).astype(F32)
    raise ValueError(kind)


def zero_sign_fixed(kind, v32):
    """Mask of inputs where the SF's IEEE result is a zero of a fixed sign."""
    v32 = np.asarray(v32)
    if kind == "RECIP":
        return np.isinf(v32)
    if kind == "TANH":
        return v32 == 0
    return np.zeros(v32.shape, bool)


_TWO128 = 2.0 ** 128


def ulp_diff(got32, want):
    """|got - want| in fp32 ulps of want, elementwise, for elements where both are numbers and want
    is finite (others: 0 here; same() compares their class).  The ulp of want is that of the fp32
    binade it lies in, 2^-149 for a denormal or zero want, 2^104 in the last binade; an infinite got
    and a want past FLT_MAX both count as 2^128, one ulp step above FLT_MAX."""
    got = np.asarray(got32).astype(np.float64)
    want = np.asarray(want, np.float64)
    ok = np.isfinite(want) & ~np.isnan(got)
    g = np.where(np.isinf(got), np.sign(got) * _TWO128, got)
    w = np.clip(np.where(ok, want, 0.0), -_TWO128, _TWO128)   # past FLT_MAX every value rounds to inf
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(w), 2.0 ** -126)))
    e = np.clip(e, -126, 127)
    ulp = 2.0 ** (e - 23)
    return np.where(ok, np.abs(np.where(ok, g, 0.0) - w) / ulp, 0.0)


def same(got32, want, ulps=0.0, zero_sign=False):
    """Boolean mask: got32 agrees with want (fp64, or fp32 for exact results).  See the module
    docstring.  zero_sign: False, True, or a mask of elements whose zero sign must match."""
    got = np.asarray(got32)
    assert got.dtype == F32
    want = np.asarray(want, np.float64)
    g64 = got.astype(np.float64)
    nan_g, nan_w = np.isnan(g64), np.isnan(want)
    inf_w = np.isinf(want)
    ok = np.where(nan_g | nan_w, nan_g & nan_w, True)
    ok &= np.where(inf_w, g64 == want, True)          # same infinity, with sign
    num = ~(nan_g | nan_w | inf_w)
    ok &= np.where(num, ulp_diff(got, want) <= ulps, True)
    zs = np.broadcast_to(np.asarray(zero_sign, bool), got.shape)
    both0 = num & (g64 == 0) & (want == 0)
    ok &= np.where(both0 & zs, np.signbit(g64) == np.signbit(want), True)
    return ok


def bits_same(a32, b32):
    """Boolean mask: equal bits, or both NaN (any payload)."""
    a, b = np.ascontiguousarray(a32), np.ascontiguousarray(b32)
    assert a.dtype == F32 and b.dtype == F32 and a.shape == b.shape
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def describe(mask_ok, inputs, got, want, limit=6):
    """A short list of the failing (input, got, want) triples for an assertion message."""
    bad = np.flatnonzero(~np.asarray(mask_ok).ravel())
    inp, got, want = np.asarray(inputs).ravel(), np.asarray(got).ravel(), np.asarray(want).ravel()
    rows = [f"in={inp[i % inp.size]!r} got={got[i]!r} want={want[i]!r}" for i in bad[:limit]]
    return f"{bad.size} mismatches: " + "; ".join(rows)


def bin_probes():
    """The 24 values of PROBES whose cross product (576 pairs) the binary ops run on."""
    v = [0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, FLT_MIN, -FLT_MIN, 1.0, -1.0, FLT_MAX, -FLT_MAX,
         np.inf, -np.inf, QNAN, 2.0 ** -127, 2.0 ** 126, 2.0 ** 127, -2.0 ** 127, 9.0, 1e-4, -9.02, 16.6,
         2.0 ** -12, -17.4]
    out = np.array(v, F32)
    assert len(out) == 24
    return out
