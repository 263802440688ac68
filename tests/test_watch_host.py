"""Host tests of the alert path: the numpy model of cc_watch_match against a literal restatement of the reference's loop
(clearcam.py:1289-1307), AlertBook's bookkeeping with an injected numpy matcher, and the binding's symbol list.  No GPU."""
import numpy as np
import pytest

import watch_cases as wc
from clearcam_amd import _lib
from clearcam_amd.alerts import AlertBook, camera_of


def reference_walk(S, thr, alert_group, crop_group, armed, now=1000.0):
    """The reference's loop, literally: for each crop, the alerts of its camera in dict order; skip when `now - last_det < 60` or
    the alert is not active; the first with `similarity > threshold` notifies, takes `last_det = now` and the walk breaks."""
    B, A = S.shape
    by_cam = {}
    for a in range(A):
        by_cam.setdefault(int(alert_group[a]), {})[a] = {"last_det": 0.0, "active": armed is None or bool(armed[a]), "threshold": float(thr[a])}
    alert, score = [-1] * B, [0.0] * B
    for b in range(B):
        alerts = by_cam.get(int(crop_group[b]), {})
        for k, v in alerts.items():
            if now - v["last_det"] < 60 or not v["active"]:
                continue
            similarity = float(S[b, k])
            if similarity > v["threshold"]:
                alerts[k]["last_det"] = now
                alert[b], score[b] = k, similarity
                break
    return np.asarray(alert, np.int32), np.asarray(score, np.float32)


@pytest.mark.parametrize("seed", wc.SEEDS)
@pytest.mark.parametrize("shape", wc.WORLDS)
def test_resolve_model_is_the_reference_walk(shape, seed):
    w = wc.world(*shape, seed)
    S = wc.product64(w.E, w.D)
    thr = wc.median_thresholds(S, w.alert_group, w.crop_group)
    for armed in (w.armed, None):
        alert, score = wc.resolve(S, thr, w.alert_group, w.crop_group, armed)
        ref_alert, ref_score = reference_walk(S, thr, w.alert_group, w.crop_group, armed)
        assert np.array_equal(alert, ref_alert) and np.array_equal(score, ref_score)
    alert, _ = wc.resolve(S, thr, w.alert_group, w.crop_group, w.armed)
    fired, later = wc.check_not_vacuous(S, thr, w, w.armed, alert)
    print(f"world {shape} seed {seed}: {fired} of {int(w.armed.sum())} armed alerts fired, {later} crops received a later alert, "
          f"{int((alert < 0).sum())} crops fired nothing")


def test_resolve_model_strictness_and_nan():
    S = np.array([[0.5, 0.5], [np.nan, 0.9], [0.6, 0.5]], np.float32)
    thr = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(-np.inf))], np.float32)
    alert, score = wc.resolve(S, thr, [0, 0], [0, 0, 0], None)
    assert alert.tolist() == [1, -1, 0] and score.tolist() == [0.5, 0.0, np.float32(0.6)]   # 0.5 > 0.5 is false; NaN never hits; row 1's 0.9: alert 1 is spent


def _matcher(book):
    """A numpy matcher with WatchList.match's signature over the book's own table."""
    calls = []

    def match(embs, crop_groups, armed=None):
        desc, thr, grp = book.table()
        calls.append((np.asarray(crop_groups).copy(), None if armed is None else np.asarray(armed).copy()))
        return wc.resolve(wc.product64(np.asarray(embs, np.float32), desc), thr, grp, crop_groups, armed)
    match.calls = calls
    return match


def _onehot(i, dim=8):
    v = np.zeros(dim, np.float32); v[i] = 1.0
    return v


def _path(cam, i):
    return f"data/cameras/{cam}/objects/2026-01-01/{1000 + i}.0_{i}_0.jpg"


def test_camera_of_takes_the_component_after_cameras():
    assert camera_of("data/cameras/front door/objects/2026-01-01/1.0_2_0.jpg") == "front door"
    assert camera_of("C:\\nvr\\cameras\\gate\\objects\\x.jpg") == "gate"
    assert camera_of("nowhere/x.jpg") is None and camera_of("data/cameras") is None


def test_alert_book_cooldown_rearms_exactly_at_60_s():
    book = AlertBook(dim=8)
    book.set_camera("gate", {"van": {"desc": "a van", "desc_emb": _onehot(0), "threshold": 0.5}})
    match = _matcher(book)
    e = _onehot(0)[None]
    assert book.armed(1000.0).tolist() == [1]
    assert book.check(match, e, [_path("gate", 0)], now=1000.0) == [(_path("gate", 0), "gate", "van", "a van", 1.0)]
    assert book.cams["gate"]["van"].last_det == 1000.0
    for now in (1000.0, 1030.0, 1059.999):
        assert book.armed(now).tolist() == [0]
        assert book.check(match, e, [_path("gate", 1)], now=now) == []
    assert book.armed(1060.0).tolist() == [1]                               # the reference skips on `< 60`: 60 s sharp re-arm
    assert len(book.check(match, e, [_path("gate", 2)], now=1060.0)) == 1
    assert book.armed(1119.0).tolist() == [0] and book.armed(1120.0).tolist() == [1]


def test_alert_book_never_arms_inactive_or_undescribed_alerts():
    book = AlertBook(dim=8)
    switch = {"on": False}
    book.set_camera("gate", {
        "off": {"desc": "x", "desc_emb": _onehot(0), "threshold": 0.5, "active": False},
        "callable": {"desc": "y", "desc_emb": _onehot(0), "threshold": 0.5, "active": lambda: switch["on"]},
        "motion only": {"desc": None, "threshold": 0.5},
        "live": {"desc": "z", "desc_emb": _onehot(0)},
    })
    assert book.armed(1000.0).tolist() == [0, 0, 0, 1]
    assert book.cams["gate"]["live"].threshold == 0.28                      # the reference's default
    match = _matcher(book)
    got = book.check(match, _onehot(0)[None], [_path("gate", 0)], now=1000.0)
    assert [(g[2], g[3]) for g in got] == [("live", "z")]
    switch["on"] = True
    assert book.armed(1000.0).tolist() == [0, 1, 0, 0]                      # `live` is cooling down now
    assert [g[2] for g in book.check(match, _onehot(0)[None], [_path("gate", 1)], now=1000.0)] == ["callable"]


def test_alert_book_priority_is_the_mapping_order_and_cameras_never_cross():
    book = AlertBook(dim=8)
    # both cameras describe the same thing; `yard` lists its alerts the other way round
    book.set_camera("gate", {"b": {"desc": "B", "desc_emb": _onehot(1), "threshold": 0.5}, "a": {"desc": "A", "desc_emb": _onehot(1), "threshold": 0.5}})
    book.set_camera("yard", {"a": {"desc": "A", "desc_emb": _onehot(1), "threshold": 0.5}, "b": {"desc": "B", "desc_emb": _onehot(1), "threshold": 0.5}})
    assert [(c, k) for c, k, _ in book.flat()] == [("gate", "b"), ("gate", "a"), ("yard", "a"), ("yard", "b")]
    assert book.table()[2].tolist() == [0, 0, 1, 1]
    match = _matcher(book)
    paths = [_path("yard", 0), _path("gate", 1), _path("gate", 2), _path("gate", 3), _path("street", 4), _path("yard", 5)]
    assert book.crop_groups(paths).tolist() == [1, 0, 0, 0, -1, 1]
    embs = np.stack([_onehot(1)] * 6)
    got = book.check(match, embs, paths, now=500.0)
    # crop order; within a camera the mapping's order; the third gate crop finds both spent; `street` has no alerts
    assert [(g[0], g[1], g[2]) for g in got] == [(paths[0], "yard", "a"), (paths[1], "gate", "b"), (paths[2], "gate", "a"), (paths[5], "yard", "b")]
    assert all(g[4] == 1.0 for g in got) and len(match.calls) == 1           # one matcher call for the batch
    assert {(c, k): a.last_det for c, k, a in book.flat()} == {("gate", "b"): 500.0, ("gate", "a"): 500.0, ("yard", "a"): 500.0, ("yard", "b"): 500.0}
    v = book.version
    book.remove_camera("yard")
    assert book.version != v and len(book) == 2
    assert book.crop_groups([_path("yard", 9)]).tolist() == [1]              # the number stays reserved and matches no alert
    assert book.check(match, _onehot(1)[None], [_path("yard", 9)], now=10_000.0) == []


def test_alert_book_apply_returns_crop_order_and_refuses_a_wrong_width():
    book = AlertBook(dim=8)
    book.set_camera("gate", {1: {"desc": "one", "desc_emb": _onehot(0)}, 2: {"desc": "two", "desc_emb": _onehot(1)}})
    paths = [_path("gate", i) for i in range(4)]
    got = book.apply([1, -1, 0, -1], np.array([0.7, 0.0, 0.4, 0.0], np.float32), paths, now=77.0)
    assert got == [(paths[0], "gate", 2, "two", float(np.float32(0.7))), (paths[2], "gate", 1, "one", float(np.float32(0.4)))]
    assert [a.last_det for _, _, a in book.flat()] == [77.0, 77.0]
    with pytest.raises(ValueError):
        book.set_camera("yard", {1: {"desc": "x", "desc_emb": np.zeros(5, np.float32)}})
    assert [k for _, k, _ in AlertBook(dim=8).missing()] == []
    book.set_camera("yard", {"later": {"desc": "not encoded yet"}})
    assert [(c, k) for c, k, _ in book.missing()] == [("yard", "later")] and book.armed(1000.0).tolist() == [1, 1, 0]


def test_binding_lists_the_watch_symbols():
    names = ["cc_watch_create", "cc_watch_set", "cc_watch_size", "cc_watch_scores", "cc_watch_match", "cc_watch_destroy"]
    assert all(n in _lib.SYMBOLS for n in names)                             # with the handle type `cc_watch`: the header's seven names
    hdr = open(__import__("os").path.join(wc.__file__.rsplit("tests", 1)[0], "include", "clearcam_hip.h")).read()
    assert "typedef struct cc_watch cc_watch;" in hdr and "#define CC_WATCH_MAX_ALERTS 2048" in hdr
