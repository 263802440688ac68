"""The single-launch cases of tests/epilogue_cases.py cover what the production plans reach - K loop included, at the plans' own depth.

With the route log on (cc_dev_set("route_log", 1)) every conv / GEMM launch records the kernel the selector chose, what decides its
epilogue and what picks its K loop.  AdaFace, BlazeFace and CLIP L/14 are built and run once per batch size in f16 and bf16.  Every
EXTENDED route key they log - the eleven fields of epilogue_cases plus split, simple, two, cprw, ns (tests/plan_route_cases.py) - must be
one a single-launch case reaches, or be merged into one, with the reason, in plan_route_cases.MERGED (a merge never crosses the kernel,
the tile, the planes, the residual kind, f32 output, `ns` or `act`).  The deepest case of a key must run at least min(S_plan, 2 ns + 1) K
steps, S_plan computed from the log.  The table of what the plans log is committed (tests/plan_route_table.py) so that
tests/test_plan_route_cases_host.py can hold the cases to it without a device; here it must equal the log.
The selector picks by M = B Ho Wo, so the log at B = 1 must differ from the log at the largest batch - otherwise the log does not see it.
"""
import ctypes as C

import numpy as np
import pytest

import epilogue_cases as ec
import plan_route_cases as prc
from clearcam_amd import _lib
from clearcam_amd.arch import CLIP_L14
from clearcam_amd.weights import synthetic_adaface_state_dict, synthetic_blazeface_state_dict, synthetic_clip_state_dict

pytestmark = pytest.mark.gpu
NREC = _lib.ROUTE_REC_INTS
NHEAD = len(ec.KEY_FIELDS)                              # a record: the eleven fields, the layer's seven-int shape, then split, simple, two, cprw, ns


def take_log():
    """Read and clear the route log: {extended route key: the set of (B, H, W, Cin, Cout, Ho, Wo) of the layers that logged it}."""
    cap = 1 << 12
    buf = (C.c_int * (cap * NREC))()
    out = {}
    while True:                                          # records that do not fit stay in the log for the next call
        n = C.c_int(0)
        _lib.check(_lib.lib().cc_route_log_take(buf, cap, C.byref(n)))
        got = min(n.value, cap)
        for r in np.frombuffer(buf, np.int32, got * NREC).reshape(got, NREC):
            key = tuple(int(v) for v in r[:NHEAD]) + tuple(int(v) for v in r[NHEAD + 7:])
            out.setdefault(key, set()).add(tuple(int(v) for v in r[NHEAD:NHEAD + 7]))
        if n.value <= cap:
            return out


@pytest.fixture(scope="module")
def weights():
    return {"adaface": synthetic_adaface_state_dict(777), "blazeface": synthetic_blazeface_state_dict(555),
            "clip": synthetic_clip_state_dict(CLIP_L14, 4321)}


@pytest.fixture(scope="module")
def clip_handles(weights):
    """One CLIP L/14 handle per dtype, made on first use, serves the image and the text plan (loading it is the slow part)."""
    from clearcam_amd.objects import OpenCLIP
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = OpenCLIP(state_dict=weights["clip"], arch=CLIP_L14, dtype=dtype)
        return made[dtype]
    yield get
    for m in made.values():
        m.close()


# each maker returns (run(B), close())
def _adaface(weights, clip_handles, dtype):
    from clearcam_amd.adaface import ADAFACE
    m = ADAFACE(state_dict=weights["adaface"], dtype=dtype)
    rng = np.random.default_rng(3)
    return (lambda B: m.embed_batch(rng.integers(0, 256, (B, 112, 112, 3), dtype=np.uint8))), m.close


def _blazeface(weights, clip_handles, dtype):
    from clearcam_amd.blazeface import BlazeFace
    m = BlazeFace(state_dict=weights["blazeface"], dtype=dtype)
    rng = np.random.default_rng(4)
    return (lambda B: m.detect_batch(rng.integers(0, 256, (B, 640, 640, 3), dtype=np.uint8))), m.close


def _clip_image(weights, clip_handles, dtype):
    m = clip_handles(dtype)
    rng = np.random.default_rng(5)
    return (lambda B: m.precompute_embedding(rng.standard_normal((B, 3, 224, 224), dtype=np.float32))), (lambda: None)


def _clip_text(weights, clip_handles, dtype):
    m = clip_handles(dtype)
    rng = np.random.default_rng(6)

    def run(B):
        t = np.zeros((B, CLIP_L14.t_ctx), np.int32)
        t[:, 0], t[:, 1:9], t[:, 9] = 49406, rng.integers(1000, 40000, (B, 8)), 49407
        return m.encode_tokens(t)
    return run, (lambda: None)


PLANS = [("adaface", _adaface, (1, 3, 12, 40, 256)), ("blazeface", _blazeface, (1, 32)),
         ("clip_image", _clip_image, (1, 8, 64, 255)), ("clip_text", _clip_text, (1, 8, 64))]     # 255: bench.py's batch
assert tuple(p[0] for p in PLANS) == prc.PLANS


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_every_route_of_the_plan_has_a_single_launch_case(plan, dtype, weights, clip_handles):
    name, make, batches = plan
    L = _lib.lib()
    covered = prc.covered_cases()
    for k, (to, why) in prc.MERGED.items():
        assert k not in covered and to in covered and why.strip() and prc.merge_is_legal(k, to), ("a merged key needs a covered key it may merge into and a reason", k)
    logs = {}
    run, close = make(weights, clip_handles, dtype)
    try:
        _lib.check(L.cc_dev_set(b"route_log", 1))
        take_log()
        # A plan is built at the first call with a batch size: its launches run once eagerly and once under graph capture, and that is
        # when they are logged (a graph replay calls no launcher).  Every batch size below is new to the handle, so every run(B) logs.
        for B in batches:
            run(B)
            logs[B] = take_log()
    finally:
        _lib.check(L.cc_dev_set(b"route_log", 0))
        take_log()
        close()
    assert all(logs[B] for B in batches), (name, "no conv launch was logged", {B: len(v) for B, v in logs.items()})
    table = prc.table_of(logs)                            # extended key -> (deepest Ktot, batch, shape): S_plan comes from it
    direct, merged, missing, shallow = prc.audit(table, covered)
    print(f"{name} {dtype}: " + ", ".join(f"B={B}: {len(logs[B])} keys" for B in batches)
          + f"; {len(table)} extended keys: {len(direct)} covered directly, {len(merged)} merged, {len(missing)} missing, {len(shallow)} too shallow")
    lines = [f"  {prc.describe(k)}   deepest at batch {table[k][1]}: K = {table[k][0]}, B,H,W,Cin,Cout,Ho,Wo = {table[k][2]}" for k in missing]
    assert not missing, f"{name} {dtype}: {len(missing)} extended route keys no single-launch case reaches:\n" + "\n".join(lines)
    lines = [f"  {prc.describe(k)}   the plan runs K = {table[k][0]}: {need} K steps asked, the deepest case ({who}) runs {have}" for k, need, have, who in shallow]
    assert not shallow, f"{name} {dtype}: {len(shallow)} extended route keys whose deepest case is too shallow:\n" + "\n".join(lines)
    assert table == prc.TABLE[name], (f"{name} {dtype}: tests/plan_route_table.py is not what the plan logs; this is:\n" + prc.format_table({name: table}))
    assert set(logs[batches[0]]) != set(logs[batches[-1]]), (name, "the log is the same at B = 1 and at the largest batch: it does not see the selector")
