"""Every refusal of gta_reduce and gta_reduce_multi: return code, full gta_last_error() text, order.

The host code checks its arguments before any device work, so the calls run without a GPU: the
pointers are fake non-NULL addresses that no check dereferences (ys / ldys of gta_reduce_multi are
real host arrays: the output-array checks read them).  EVERY call below carries at least one fault
or n_rows == 0, so none reaches a launch.  A case is a set of overrides of a valid call; the cases
with two faults pin the order of adjacent checks (the earlier check's text must come back).
"""
import ctypes

import pytest

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _build, _lib

P = 0x10000  # a fake device address, 64 KiB aligned
BIG = 2 ** 31  # INT32_MAX + 1
ARG, UNS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
EDGE, SRC, DST = _lib.IDX_EDGE, _lib.IDX_SRC, _lib.IDX_DST
ALL5 = _lib.MR_MEAN | _lib.MR_MAX | _lib.MR_MIN | _lib.MR_VAR | _lib.MR_STD

VALID = dict(indptr=P, indices=P, n_rows=10, nnz=20, x_mode=SRC, x=P, ldx=8, F=8, x_dtype=_lib.GTA_F32,
             plan=None, chunk=0, ws=None)
VALID_REDUCE = dict(VALID, red=_lib.RED_MAX, y=P, ldy=8)
VALID_MULTI = dict(VALID, which=_lib.MR_MEAN | _lib.MR_MAX, ys=(P, P), ldys=(8, 8), eps=1e-5)

BAD_SIZES, BAD_MODE, BAD_DTYPE = dict(F=0), dict(x_mode=3), dict(x_dtype=2)
BF16_EDGE = dict(x_dtype=_lib.GTA_BF16, x_mode=EDGE)
F_BIG = dict(F=BIG, ldx=BIG, ldy=BIG, ldys=(BIG, BIG))
NO_INDICES = dict(indices=None)
PLAN_BARE = dict(plan=P)


@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def call_reduce(lib, over):
    a = dict(VALID_REDUCE, **over)
    a.pop("ldys", None)
    rc = lib.gta_reduce(a["red"], a["indptr"], a["indices"], a["n_rows"], a["nnz"], a["x_mode"], a["x"], a["ldx"],
                        a["F"], a["x_dtype"], a["y"], a["ldy"], a["plan"], a["chunk"], a["ws"], None)
    return rc, lib.gta_last_error().decode()


def call_multi(lib, over):
    a = dict(VALID_MULTI, **over)
    a.pop("ldy", None)
    ys = None if a["ys"] is None else (ctypes.c_void_p * len(a["ys"]))(*a["ys"])
    ldys = None if a["ldys"] is None else (ctypes.c_int64 * len(a["ldys"]))(*a["ldys"])
    rc = lib.gta_reduce_multi(a["which"], a["indptr"], a["indices"], a["n_rows"], a["nnz"], a["x_mode"], a["x"],
                              a["ldx"], a["F"], a["x_dtype"], ys, ldys, a["eps"], a["plan"], a["chunk"], a["ws"], None)
    return rc, lib.gta_last_error().decode()


def merged(*overs):
    out = {}
    for o in overs:
        out.update(o)
    return out


R_RED = "reduce: red must be GTA_RED_ADD, GTA_RED_MAX or GTA_RED_MIN"
R_BF16 = "{}: bf16 rows are gathered by index (SRC / DST)"
R_DTYPE = "{}: x_dtype must be F32 or BF16"
R_PLAN = "{}: plan needs chunk and workspace"
M_WHICH = "reduce_multi: which must be a non-empty set of GTA_MR_* bits"
M_YS = "reduce_multi: ys / ldys is NULL"
M_OUT = "reduce_multi: an output is NULL or its row stride < F"


def common_single(who):
    """The refusals both entry points give, as (id, overrides, code, text)."""
    return [
        ("sizes-n_rows", dict(n_rows=-1), ARG, f"{who}: bad sizes"),
        ("sizes-nnz", dict(nnz=-1), ARG, f"{who}: bad sizes"),
        ("sizes-F", BAD_SIZES, ARG, f"{who}: bad sizes"),
        ("x_mode-3", BAD_MODE, ARG, f"{who}: bad x_mode"),
        ("x_mode-neg", dict(x_mode=-1), ARG, f"{who}: bad x_mode"),
        ("x_dtype-2", BAD_DTYPE, ARG, R_DTYPE.format(who)),
        ("x_dtype-neg", dict(x_dtype=-1), ARG, R_DTYPE.format(who)),
        ("bf16-edge", BF16_EDGE, UNS, R_BF16.format(who)),
        ("F-large", F_BIG, UNS, f"{who}: F too large"),
        ("indptr-null", dict(indptr=None), ARG, f"{who}: bad arguments"),
        ("x-null-with-edges", dict(x=None), ARG, f"{who}: bad arguments"),
        ("ldx-small", dict(ldx=7), ARG, f"{who}: bad arguments"),
        ("src-no-indices", NO_INDICES, ARG, f"{who}: x_mode SRC needs indices"),
        ("plan-no-chunk", dict(plan=P, chunk=0, ws=P), ARG, R_PLAN.format(who)),
        ("plan-neg-chunk", dict(plan=P, chunk=-64, ws=P), ARG, R_PLAN.format(who)),
        ("plan-no-workspace", dict(plan=P, chunk=64, ws=None), ARG, R_PLAN.format(who)),
        # two faults: the earlier check answers
        ("sizes+x_mode", merged(BAD_SIZES, BAD_MODE), ARG, f"{who}: bad sizes"),
        ("x_mode+x_dtype", merged(BAD_MODE, BAD_DTYPE), ARG, f"{who}: bad x_mode"),
        ("x_dtype+edge", merged(BAD_DTYPE, dict(x_mode=EDGE)), ARG, R_DTYPE.format(who)),  # (bf16 needs a good dtype)
        ("x_dtype+F-large", merged(BAD_DTYPE, F_BIG), ARG, R_DTYPE.format(who)),
        ("bf16-edge+F-large", merged(BF16_EDGE, F_BIG), UNS, R_BF16.format(who)),
        ("F-large+n_rows-0", merged(F_BIG, dict(n_rows=0)), UNS, f"{who}: F too large"),
        ("bf16-edge+n_rows-0", merged(BF16_EDGE, dict(n_rows=0)), UNS, R_BF16.format(who)),
        ("x_dtype+n_rows-0", merged(BAD_DTYPE, dict(n_rows=0)), ARG, R_DTYPE.format(who)),
        ("arguments+src-no-indices", merged(dict(indptr=None), NO_INDICES), ARG, f"{who}: bad arguments"),
        ("src-no-indices+plan", merged(NO_INDICES, PLAN_BARE), ARG, f"{who}: x_mode SRC needs indices"),
        ("arguments+plan", merged(dict(ldx=7), PLAN_BARE), ARG, f"{who}: bad arguments"),
    ]


REDUCE_CASES = common_single("reduce") + [
    ("red-3", dict(red=3), ARG, R_RED),
    ("red-neg", dict(red=-1), ARG, R_RED),
    ("y-null", dict(y=None), ARG, "reduce: bad arguments"),
    ("ldy-small", dict(ldy=7), ARG, "reduce: bad arguments"),
    ("ldy-small-no-edges", dict(ldy=7, nnz=0, x=None, indices=None), ARG, "reduce: bad arguments"),
    ("red+sizes", merged(dict(red=3), BAD_SIZES), ARG, R_RED),
    # the sum is the aggregate's: its refusals come back behind the prefix
    ("add-sizes", merged(dict(red=_lib.RED_ADD), BAD_SIZES), ARG, "reduce (ADD): aggregate: bad sizes"),
    ("add-x_mode", merged(dict(red=_lib.RED_ADD), BAD_MODE), ARG, "reduce (ADD): aggregate: bad x_mode"),
    ("add-x_dtype", merged(dict(red=_lib.RED_ADD), BAD_DTYPE), ARG, "reduce (ADD): aggregate: x_dtype must be F32 or BF16"),
    ("add-bf16-edge", merged(dict(red=_lib.RED_ADD), BF16_EDGE), UNS,
     "reduce (ADD): aggregate: bf16 rows are gathered by index (SRC / DST) with head weights or none"),
    ("add-F-large", merged(dict(red=_lib.RED_ADD), F_BIG), UNS, "reduce (ADD): aggregate: F too large"),
    ("add-y-null", dict(red=_lib.RED_ADD, y=None), ARG, "reduce (ADD): aggregate: bad arguments"),
    ("add-src-no-indices", merged(dict(red=_lib.RED_ADD), NO_INDICES), ARG,
     "reduce (ADD): aggregate: x_mode SRC needs indices"),
    ("add-plan", merged(dict(red=_lib.RED_ADD), PLAN_BARE), ARG, "reduce (ADD): aggregate: plan needs chunk and workspace"),
]

MULTI_CASES = common_single("reduce_multi") + [
    ("which-empty", dict(which=0), ARG, M_WHICH),
    ("which-stray-bit", dict(which=32 | _lib.MR_MAX), ARG, M_WHICH),
    ("which-neg", dict(which=-1), ARG, M_WHICH),
    ("ys-null", dict(ys=None), ARG, M_YS),
    ("ldys-null", dict(ldys=None), ARG, M_YS),
    ("output-null-first", dict(ys=(None, P)), ARG, M_OUT),
    ("output-null-last", dict(which=ALL5, ys=(P, P, P, P, None), ldys=(8,) * 5), ARG, M_OUT),
    ("output-ld-small", dict(ldys=(8, 7)), ARG, M_OUT),
    ("which+sizes", merged(dict(which=0), BAD_SIZES), ARG, M_WHICH),
    ("F-large+ys-null", merged(F_BIG, dict(ys=None)), UNS, "reduce_multi: F too large"),
    ("ys-null+n_rows-0", dict(ys=None, n_rows=0), ARG, M_YS),
    ("ldys-null+output-null", dict(ldys=None, ys=(None, P)), ARG, M_YS),
    ("output-null+n_rows-0", dict(ys=(P, None), n_rows=0), ARG, M_OUT),
    ("output-ld-small+n_rows-0", dict(ldys=(7, 8), n_rows=0), ARG, M_OUT),
    ("output-null+arguments", dict(ys=(P, None), indptr=None), ARG, M_OUT),
]


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("case", REDUCE_CASES, ids=_ids(REDUCE_CASES))
def test_reduce_refuses(lib, case):
    _, over, code, text = case
    assert call_reduce(lib, over) == (code, text)


@pytest.mark.parametrize("case", MULTI_CASES, ids=_ids(MULTI_CASES))
def test_reduce_multi_refuses(lib, case):
    _, over, code, text = case
    assert call_multi(lib, over) == (code, text)


def test_no_rows_is_ok_before_the_pointer_checks(lib):
    """n_rows == 0 returns GTA_OK after the size / mode / dtype / F checks (cases above) and before
    the pointer checks: no pointer is looked at -- for gta_reduce_multi none but ys / ldys and the
    outputs they list, which are checked first (cases above)."""
    nothing = dict(n_rows=0, nnz=0, indptr=None, indices=None, x=None, ldx=0)
    for red in (_lib.RED_MAX, _lib.RED_MIN, _lib.RED_ADD):
        assert call_reduce(lib, dict(nothing, red=red, y=None, ldy=0))[0] == _lib.OK
    assert call_reduce(lib, dict(nothing, plan=P))[0] == _lib.OK
    assert call_multi(lib, nothing)[0] == _lib.OK
    assert call_multi(lib, dict(nothing, plan=P))[0] == _lib.OK
