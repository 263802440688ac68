"""The AdaFace, BlazeFace and CLIP L/14 plans against their CPU oracles at the batch sizes where the selector picks new kernels.

The conv / GEMM selector picks by M = B Ho Wo (tests/plan_route_table.py: the 128 x 128, 256 x 256, persistent and phase routes appear at
B = 12, 40, 256 for AdaFace and at B = 8, 64 for CLIP), and every other end-to-end comparison with an oracle runs at B <= 5.  Here a batch
of production size is built from four distinct inputs (tests/batch_cases.py), so the oracle costs four evaluations per model, and for
every (plan, dtype, B):
  routes   with the route log on, the first call at B (it builds and captures the plan) logs only keys of plan_route_cases.TABLE[plan] -
           routes a single-launch case vouches for - and at least one key the model's small oracle batch did not log.  The table holds
           the 16-bit plans; the f32 selector takes none of its M-dependent branches (conv_mfma.hip choose_conv: all of them stand under
           `dt != F32`), so an f32 plan must log the SAME keys at B as at the small batch, which is asserted instead: the f32 cases hold
           the arenas, the attention grid and the per-row kernels at B tokens rows, and the ragged last tile of the 128-row kernel;
  bars     check_rows: every row meets the model's own parity bar against the oracle row of its input, and all copies of an input are
           bit-equal (a swapped, shifted or neighbour-contaminated row breaks that even where a 16-bit cosine bar cannot tell);
  replay   the second call at B (a graph replay) returns the first call's bits.
The worst error / bar per (plan, dtype, B) and the module's wall time (handles and oracles apart) are printed at module end."""
import time

import numpy as np
import pytest

import batch_cases as bc
import plan_route_cases as prc
from clearcam_amd import _lib
from clearcam_amd.arch import CLIP_L14
from test_gpu_plan_routes import take_log, weights          # noqa: F401  (the module-scoped weights fixture: CLIP L/14 is made once)

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
CASES = [(plan, dtype, B) for plan in prc.PLANS for dtype in DTYPES for B in bc.BATCHES[plan]]
BAR_OF = {"adaface": "adaface", "blazeface": "blazeface", "clip_image": "clip", "clip_text": "clip"}

WORST = {}                                                  # (plan, dtype, B) -> the worst error / bar over the rows
SECONDS = {"handles": 0.0, "oracles": 0.0, "weights": 0.0}
RUNS = {}                                                   # (plan, dtype, B) -> (first, second, keys logged at the small batch, keys logged at B)
SMALL_KEYS = {}                                             # (plan, dtype) -> keys logged when the small batch's plan was built


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.perf_counter()
    yield
    for (plan, dtype, B), w in sorted(WORST.items()):
        print(f"\n[plan batches] {plan} {dtype} B={B}: worst error / bar = {w:.4f}", end="")
    total = time.perf_counter() - t0
    print(f"\n[plan batches] wall time {total:.1f} s: weights {SECONDS['weights']:.1f} s, handles {SECONDS['handles']:.1f} s, "
          f"oracles {SECONDS['oracles']:.1f} s, the cases {total - sum(SECONDS.values()):.1f} s")


@pytest.fixture(scope="module")
def sd(request):
    """test_gpu_plan_routes.weights, timed."""
    t0 = time.perf_counter()
    out = request.getfixturevalue("weights")
    SECONDS["weights"] += time.perf_counter() - t0
    return out


@pytest.fixture(scope="module")
def inputs():
    """plan -> the four distinct inputs.  Shared: do not modify."""
    return {"adaface": bc.face_crops(), "blazeface": bc.blaze_images(), "clip_image": bc.clip_images(CLIP_L14.image_size),
            "clip_text": bc.text_tokens(CLIP_L14)}


@pytest.fixture(scope="module")
def want(sd, inputs):
    """plan -> the oracle's rows for the four inputs: one evaluation per model.  The separation that tests/test_batch_cases_host.py asserts
    for the light oracles is asserted here for CLIP L/14, before anything is compared.  Shared: do not modify."""
    from oracle.adaface_oracle import AdaFaceOracle
    from oracle.blazeface_oracle import BlazeFaceOracle
    from oracle.clip_oracle import OpenCLIPOracle
    t0 = time.perf_counter()
    face, blaze, clip = AdaFaceOracle(sd["adaface"]), BlazeFaceOracle(sd["blazeface"]), OpenCLIPOracle(sd["clip"], CLIP_L14)
    out = {"adaface": np.concatenate([face(f) for f in inputs["adaface"]]),
           "blazeface": np.stack([blaze(f) for f in inputs["blazeface"]]),
           "clip_image": clip.precompute_embedding(inputs["clip_image"]),
           "clip_text": clip.encode_tokens(inputs["clip_text"])}
    SECONDS["oracles"] += time.perf_counter() - t0
    for plan in ("clip_image", "clip_text", "adaface"):
        sep = bc.separation(out[plan])
        print(f"\n[plan batches] {plan}: the closest two oracle rows differ by {sep:.3g}", end="")
        assert sep > 10 * bc.F32_ABS_BAR[BAR_OF[plan]], (plan, "the oracle cannot tell two of the inputs apart", sep)
    assert all(int((d[:, 16] != 0).sum()) > 10 for d in out["blazeface"])
    return out


@pytest.fixture(scope="module")
def handles(sd):
    """get(plan, dtype): one handle per (model, dtype), made on first use; CLIP's serves the image and the text plan."""
    from clearcam_amd.adaface import ADAFACE
    from clearcam_amd.blazeface import BlazeFace
    from clearcam_amd.objects import OpenCLIP
    made = {}

    def get(plan, dtype):
        model = "clip" if plan.startswith("clip") else plan
        if (model, dtype) not in made:
            t0 = time.perf_counter()
            if model == "adaface":
                made[(model, dtype)] = ADAFACE(state_dict=sd["adaface"], dtype=dtype)
            elif model == "blazeface":
                made[(model, dtype)] = BlazeFace(state_dict=sd["blazeface"], dtype=dtype)
            else:
                made[(model, dtype)] = OpenCLIP(state_dict=sd["clip"], arch=CLIP_L14, dtype=dtype)
            SECONDS["handles"] += time.perf_counter() - t0
        return made[(model, dtype)]
    yield get
    for m in made.values():
        m.close()


def _call(plan, m, x):
    if plan == "adaface":
        return m.embed_batch(x)
    if plan == "blazeface":
        return m.detect_batch(x)
    if plan == "clip_image":
        return m.precompute_embedding(x).numpy()
    return m.encode_tokens(x)


def run_case(plan, dtype, B, handles, inputs):
    """(first call at B, second call at B, keys logged by the small batch, keys logged at B), run once per case."""
    key = (plan, dtype, B)
    if RUNS.get(key) == "failed":                            # not run a second time: whatever stopped it is in the first test's report
        pytest.fail(f"{plan} {dtype} B={B} did not run (see the first test of this case)")
    if key not in RUNS:
        RUNS[key] = "failed"
        m, L = handles(plan, dtype), _lib.lib()
        x = np.ascontiguousarray(inputs[plan][bc.pattern(B)])
        try:
            _lib.check(L.cc_dev_set(b"route_log", 1))
            take_log()
            if (plan, dtype) not in SMALL_KEYS:              # a plan logs when it is built: the small batch's, at the handle's first case
                _call(plan, m, np.ascontiguousarray(inputs[plan][bc.pattern(bc.SMALL[plan])]))
                SMALL_KEYS[(plan, dtype)] = set(take_log())
            first = _call(plan, m, x)
            at_b = set(take_log())
        finally:
            _lib.check(L.cc_dev_set(b"route_log", 0))
            take_log()
        second = _call(plan, m, x)
        RUNS[key] = (np.ascontiguousarray(first, dtype=np.float32), np.ascontiguousarray(second, dtype=np.float32), SMALL_KEYS[(plan, dtype)], at_b)
    return RUNS[key]


def _ids(c):
    return f"{c[0]}-{c[1]}-B{c[2]}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_batch_runs_the_routes_it_means_to(case, handles, inputs):
    plan, dtype, B = case
    _, _, small, at_b = run_case(plan, dtype, B, handles, inputs)
    assert small and at_b, (case, "no conv launch was logged: the plan was not built by this call", len(small), len(at_b))
    if dtype == "f32":
        assert at_b == small, (f"{plan} f32: the selector chose by the batch size; these keys are new at B = {B}:\n"
                               + "\n".join("  " + prc.describe(k) for k in sorted(at_b ^ small)))
        return
    new = at_b - small
    print(f"{plan} {dtype} B={B}: {len(at_b)} keys, {len(new)} of them not logged at B={bc.SMALL[plan]}")
    assert new, (case, f"B = {B} logs no route that B = {bc.SMALL[plan]} did not: the batch does not reach the routes it is here for")
    outside = sorted(at_b - set(prc.TABLE[plan]))
    assert not outside, (f"{plan} {dtype} B={B} runs {len(outside)} routes tests/plan_route_table.py does not hold, so no single-launch case vouches for them "
                         f"(add the batch to test_gpu_plan_routes.PLANS and regenerate the table):\n" + "\n".join("  " + prc.describe(k) + f"   {k}" for k in outside))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_batch_holds_the_oracle_bars(case, handles, inputs, want):
    plan, dtype, B = case
    first, _, _, _ = run_case(plan, dtype, B, handles, inputs)
    assert first.shape == (B,) + want[plan].shape[1:]
    worst = bc.check_rows(first, want[plan], bc.pattern(B), bc.BARS[(BAR_OF[plan], dtype)])
    WORST[case] = worst
    print(f"{plan} {dtype} B={B}: worst error / bar = {worst:.4f}")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_second_call_replays_the_first(case, handles, inputs):
    plan, dtype, B = case
    first, second, _, _ = run_case(plan, dtype, B, handles, inputs)
    same = first.view(np.uint32) == second.view(np.uint32)
    assert same.all(), (case, f"the graph replay differs from the call that built the plan in {int((~same).sum())} words, first at row {int(np.argwhere(~same)[0][0])}")
