"""Seen before on the host: the model of tests/sightings_cases.py held to a plain double loop, the cases the inputs of the GPU tests
carry, the condition that makes the comparison with the float64 model exact, and ObjectFinder.seen_before's host logic over a stub
index whose digest / sightings are the numpy models.  No GPU."""
import numpy as np
import pytest

from digest_cases import digest_model
from sightings_cases import (DIMS, GROUPS, MAX_GROUPS, MAX_OBJECTS, SAME_AT, SMALL_GROUP_COUNTS, STORAGES, competing, double_loop, object_sets,
                             pair_values, sightings_model, stored, threshold_margins, world)
from where_cases import passing, unit


def same(got, want, what):
    assert len(got) == len(want) == 5, what
    for name, g, x in zip(("count", "best_row", "best_score", "group_counts", "total"), got, want):
        if x is None or name == "total":
            assert g == x or (g is None and x is None), (what, name, g, x)
            continue
        assert g.dtype == x.dtype and g.shape == x.shape, (what, name, g.dtype, x.dtype, g.shape, x.shape)
        assert np.array_equal(g.view(np.uint32) if name == "best_score" else g, x.view(np.uint32) if name == "best_score" else x), (what, name)


def test_the_abi_knows_the_entry_point_and_the_constants():
    from clearcam_amd import _lib
    assert "cc_index_sightings" in _lib.SYMBOLS
    assert (_lib.SIGHT_MAX_OBJECTS, _lib.SIGHT_MAX_GROUPS, _lib.SIGHT_SKIP_SELF) == (MAX_OBJECTS, MAX_GROUPS, 1) == (1024, 4096, 1)


@pytest.mark.parametrize("dim", DIMS)
def test_the_model_is_the_double_loop(dim):
    w = world(dim)
    D = stored(w.E, "f32")
    rng = np.random.default_rng(dim)
    picks = [np.arange(150), np.arange(100, 260), np.sort(rng.choice(w.n, 170, replace=False)), np.arange(1), np.arange(0)]
    for comp in picks:
        values = {}
        for n in (1, 3, 70):
            plain = rng.choice(260, n, replace=False)
            repeats = plain.copy()
            repeats[1::2] = repeats[0::2][:len(repeats[1::2])]
            for rows in (plain, repeats):
                for skip_self in (False, True):
                    ats = SAME_AT + (np.inf, -np.inf)
                    for ngc in (SMALL_GROUP_COUNTS,) if n == 70 else (0, SMALL_GROUP_COUNTS, GROUPS):
                        want = double_loop(D, rows, comp, ats, skip_self, w.group, ngc, values)
                        for same_at, x in zip(ats, want):
                            same(sightings_model(D, rows, comp, same_at, skip_self, w.group, ngc), x, (dim, len(comp), n, skip_self, same_at, ngc))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_the_inputs_carry_the_cases(dim, storage):
    w = world(dim)
    D = stored(w.E, storage)
    rows = object_sets(w, 65)
    assert len(set(rows.tolist())) < len(rows)                                         # repeats
    counts, ties, beyond = [], 0, 0
    for name in (None, "ts", "both+allowed"):
        comp, _ = competing(w, name)
        if name is not None:
            assert not np.isin(rows, comp).all()                                       # objects outside the competing set
        G = pair_values(D, rows, comp)
        for skip_self in (False, True):
            c, br, bs, gc, _ = sightings_model(D, rows, comp, SAME_AT[-1], skip_self, w.group, SMALL_GROUP_COUNTS, G=G)
            counts.extend(c.tolist())
            beyond += int((c.astype(np.int64) - gc.sum(axis=1)).sum())
            top = (G.view(np.uint32) == bs.view(np.uint32)[:, None]) & ((comp[None, :] != rows[:, None]) | (not skip_self))
            for i in np.flatnonzero(top.sum(axis=1) > 1):                              # the lowest row wins; ties between byte-equal rows are counted
                at = comp[top[i]]
                assert br[i] == at.min()
                ties += int((w.E[at].view(np.uint32) == w.E[at[0]].view(np.uint32)).all())
    assert min(counts) == 0 and max(counts) >= 40 and any(0 < c < 40 for c in counts)
    assert ties > 0 and beyond > 0


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_no_pair_comes_near_a_threshold_of_the_sightings(dim, storage):
    """Re-asserts test_no_pair_of_stored_rows_comes_near_a_threshold of tests/test_index_distinct_host.py for the thresholds used here:
    every object of the full-world cases is a row of the world, so the margins over all pairs of stored rows cover every object -
    competing pair."""
    margins, bound = threshold_margins(stored(world(dim).E, storage), SAME_AT)
    assert bound < 1e-4
    for same_at, m in zip(SAME_AT, margins):
        assert m > 10 * bound, (dim, storage, same_at, m, bound)


# ---- ObjectFinder.seen_before over a stub index ---------------------------------------------------------------------------------------
CAMS, DAYS = ("back", "front", "gate"), ("2026-01-01", "2026-01-02", "2026-01-03")


class StubIndex:
    """digest / sightings as the numpy models, over rows held on the host"""

    def __init__(self, E, group, ts, cls):
        self.D, self.group, self.ts, self.cls, self.dim = np.asarray(E, np.float32), np.asarray(group), np.asarray(ts), np.asarray(cls), E.shape[1]
        self.calls = []

    def _competing(self, allowed, ts_range, classes):
        ok = passing(self.ts, self.cls, ts_range, classes)
        if allowed is not None:
            al = np.zeros(int(self.group.max()) + 1, np.uint8)
            al[:len(allowed)] = np.asarray(allowed)[:len(al)]
            ok &= al[self.group].astype(bool)
        return np.flatnonzero(ok)

    def digest(self, same_at, start, count, allowed=None, ts_range=None, classes=None, max_leaders=1024, by="count"):
        return digest_model(self.D, self._competing(allowed, ts_range, classes), same_at, max_leaders, by, start, count, ts=self.ts)[:5]

    def sightings(self, rows, same_at=0.9, allowed=None, ts_range=None, classes=None, skip_self=False, group_counts=0, with_total=True):
        self.calls.append((list(rows), np.asarray(allowed).copy(), classes, group_counts))
        return sightings_model(self.D, rows, self._competing(allowed, ts_range, classes), same_at, skip_self, self.group, group_counts)


def stub_finder(tmp_path):
    """Today = (front, DAYS[2]).  A van seen today, on DAYS[0] at back and gate and on DAYS[1] at back; a postman seen today and on
    DAYS[1] at front; a stranger seen today only (three crops); a cat in the history only; unrelated crops everywhere."""
    from clearcam_amd.objects import ObjectFinder, _RowTable
    rng = np.random.default_rng(5)
    things = {k: unit(rng.standard_normal(64)) for k in ("van", "postman", "stranger", "cat")}
    spec = []                                                                          # (cam, day, ts, class, thing or None)
    for cam in CAMS:
        for day in DAYS:
            spec += [(cam, day, 100 + 10 * i, 0, None) for i in range(4)]
    spec += [("front", DAYS[2], 500, 2, "van"), ("front", DAYS[2], 510, 2, "van"), ("front", DAYS[2], 300, 0, "postman"),
             ("front", DAYS[2], 700 + 0, 0, "stranger"), ("front", DAYS[2], 701, 0, "stranger"), ("front", DAYS[2], 702, 0, "stranger"),
             ("back", DAYS[0], 50, 2, "van"), ("gate", DAYS[0], 60, 2, "van"), ("gate", DAYS[0], 61, 2, "van"), ("back", DAYS[1], 70, 2, "van"),
             ("front", DAYS[1], 310, 0, "postman"), ("gate", DAYS[1], 5, 7, "cat")]
    spec.sort(key=lambda s: (s[0], s[1]))                                              # folders contiguous, as ingest leaves them
    base = str(tmp_path / "cameras")
    paths, E = [], []
    for k, (cam, day, ts, c, thing) in enumerate(spec):
        paths.append(f"{base}/{cam}/objects/{day}/{ts}.0_{k}_{c}.jpg")
        E.append(unit(rng.standard_normal(64)) if thing is None else unit(things[thing] + 0.05 * unit(rng.standard_normal(64))))
    table = _RowTable()
    group = table.extend(paths)
    ts, cls = table.attrs()
    f = ObjectFinder(base)
    f._attached = True
    f._dev["store"] = (StubIndex(np.stack(E), group, ts, cls), table)
    return f, table, spec


def by_thing(entries, spec, table):
    return {spec[table.row[e[0]]][4]: e for e in entries if spec[table.row[e[0]]][4] is not None}


def test_seen_before_reports_days_cameras_and_the_new(tmp_path):
    f, table, spec = stub_finder(tmp_path)
    index = f._dev["store"][0]
    got, info = f.seen_before(cam_name="front", timestamp=DAYS[2])
    today = table.allowed("front", DAYS[2])
    rows, al, classes, ngc = index.calls[-1]
    assert ngc == len(table.dirs) and classes is None and not (al.astype(bool) & today.astype(bool)).any()      # history excludes today's folders
    assert al.sum() == len(CAMS) * len(DAYS) - 1
    assert info == {"objects": 7, "new": 5, "crops": 10, "left_over": 0, "history_crops": len(spec) - 10}
    e = by_thing(got, spec, table)
    path, n_today, t0, t1, seen, days, cams, last_day, best_path, best_score = e["van"]
    assert (n_today, t0, t1, seen, days, cams, last_day) == (2, 500, 510, 4, 2, ["back", "gate"], DAYS[1])
    assert spec[table.row[best_path]][4] == "van" and spec[table.row[best_path]][1] != DAYS[2] and best_score > 0.9
    assert e["postman"][1:8] == (1, 300, 300, 1, 1, ["front"], DAYS[1]) and "/front/objects/" + DAYS[1] in e["postman"][8]
    s = e["stranger"]
    assert s[1:8] == (3, 700, 702, 0, 0, [], None) and s[8] is not None and s[9] < 0.9 and not today[table.group[table.row[s[8]]]]
    # by="new": never seen first, most crops today first among them, then order of appearance; the seen ones behind, in the same order
    assert [x[4] == 0 for x in got] == [True] * 5 + [False] * 2 and got[0] == s and got[5] == e["van"] and got[6] == e["postman"]
    assert [table.row[x[0]] for x in got[1:5]] == sorted(table.row[x[0]] for x in got[1:5])
    first, _ = f.seen_before(cam_name="front", timestamp=DAYS[2], by="first")
    assert sorted(first) == sorted(got) and [table.row[x[0]] for x in first] == sorted(table.row[x[0]] for x in first)
    count, _ = f.seen_before(cam_name="front", timestamp=DAYS[2], by="count")
    assert [x[1] for x in count] == [3, 2, 1, 1, 1, 1, 1] and sorted(count) == sorted(got)
    digest, dinfo = f.digest(cam_name="front", timestamp=DAYS[2], by="count")
    assert [x[:4] for x in count] == digest and {k: info[k] for k in dinfo} == dinfo
    for start, n in ((0, 1), (2, 3), (6, 1), (6, 5), (7, 2), (40, 1)):                 # windows, past the end too
        assert f.seen_before(cam_name="front", timestamp=DAYS[2], start=start, count=n) == (got[start:start + n], info)


def test_seen_before_history_cam_classes_and_the_empty_cases(tmp_path):
    f, table, spec = stub_finder(tmp_path)
    index = f._dev["store"][0]
    got, info = f.seen_before(cam_name="front", timestamp=DAYS[2], history_cam="back")
    e = by_thing(got, spec, table)
    assert e["van"][4:8] == (2, 2, ["back"], DAYS[1]) and e["postman"][4:8] == (0, 0, [], None) and info["new"] == 6
    assert info["history_crops"] == sum(1 for s in spec if s[0] == "back")
    assert index.calls[-1][1].sum() == len(DAYS)
    got, info = f.seen_before(cam_name="front", timestamp=DAYS[2], classes=(2,), ts_range=(505, 600))
    assert index.calls[-1][2] == (2,) and info == {"objects": 1, "new": 0, "crops": 1, "left_over": 0, "history_crops": 4}
    assert got[0][1:8] == (1, 510, 510, 4, 2, ["back", "gate"], DAYS[1])               # ts_range narrows today, not the history
    # an empty day
    calls = len(index.calls)
    assert f.seen_before(cam_name="nowhere") == ([], {"objects": 0, "new": 0, "crops": 0, "left_over": 0, "history_crops": 0})
    assert f.seen_before(cam_name="front", timestamp=DAYS[2], ts_range=(9000, 9001)) == ([], {"objects": 0, "new": 0, "crops": 0, "left_over": 0, "history_crops": 0})
    # an empty history: everything is today (no folder filter), or the history camera has no folder
    for kw in (dict(), dict(cam_name="front", timestamp=DAYS[2], history_cam="nowhere")):
        got, info = f.seen_before(count=1000, **kw)
        digest, dinfo = f.digest(count=1000, by="count", **{k: v for k, v in kw.items() if k != "history_cam"})
        assert info == dict(dinfo, new=dinfo["objects"], history_crops=0) and len(got) == len(digest)
        assert sorted(x[:4] for x in got) == sorted(digest) and all(x[4:] == (0, 0, [], None, None, None) for x in got)
    assert len(index.calls) == calls                                                   # neither case scored anything
    for bad in (dict(by="score"), dict(start=-1), dict(count=0), dict(same_at=float("nan")), dict(ts_range=(5, 4))):
        with pytest.raises(ValueError):
            f.seen_before(**bad)
