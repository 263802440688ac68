"""ObjectFinder's ten questions over a recording stub index: which EmbeddingIndex method a question calls, with which arguments, when
the model is asked to encode a text, and what the question returns or raises - as literal values (EXPECTED), so that the layer between
the caller and the index can be rearranged without changing an answer.  No GPU and no library call.

Arrays are written as '<dtype><nested list>' strings, tuples (a `Term` too) as tuples.  An event is ("encode", text) or
(index method, positional arguments, keyword arguments), in the order they happened."""
import inspect
import sys

import numpy as np
import pytest
import torch

import clearcam_amd.objects as O
from clearcam_amd import _lib
from clearcam_amd.helpers import Tensor

DIM = 4
BASE = "/data/cameras"
NAMES = (("front", "2026-01-01", "100.0_1_0.jpg"), ("front", "2026-01-01", "110.0_1_0.jpg"), ("front", "2026-01-01", "snap.jpg"),
         ("front", "2026-01-02", "200.0_2_2.jpg"), ("back", "2026-01-01", "300.0_0_0.jpg"), ("back", "2026-01-01", "310.0_0_2.jpg"),
         ("back", "2026-01-02", "400.0_4_7.jpg"), ("back", "2026-01-02", "410.0_4_7.jpg"))
P = [f"{BASE}/{cam}/objects/{day}/{name}" for cam, day, name in NAMES]     # rows 0 .. 7: tracks 1, 1, none, 2, 0, 0, 4, 4
BAD = [f"{BASE}/gate/objects/2026-01-01/bad_name_x.jpg", f"{BASE}/gate/objects/2026-01-01/500.0_5_0.jpg"]   # rows 8, 9 of the second table
VEC = np.array([1, 0, 0, 0], np.float32)
ROWS, SCORES = [3, 0, 6], [0.875, 0.75, 0.625]                            # what every ranking of the stub answers
METHODS = ("rank", "rank_device", "rank_like", "rank_like_device", "rank_terms", "rank_terms_device", "timeline", "timeline_terms", "rank_near",
           "timeline_near", "digest", "sightings", "distinct", "distinct_device", "fetch", "scores", "search", "search_tracks")


def plain(x):
    if isinstance(x, torch.Tensor):
        x = x.numpy()
    if isinstance(x, np.ndarray):
        return f"{x.dtype}{x.tolist()}"
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, tuple):
        return tuple(plain(v) for v in x)
    if isinstance(x, list):
        return [plain(v) for v in x]
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    return x


def page(count, values, dtype, fill=-1):
    out = np.full((1, int(count)), fill, dtype)
    n = min(int(count), len(values))
    out[0, :n] = values[:n]
    return out


class Recorder:
    """Every method appends (name, args, kwargs) to `events` and returns small canned arrays of the right shape."""

    def __init__(self, n_rows, n_dirs, events):
        self.dim, self.n_rows, self.n_dirs, self.events = DIM, n_rows, n_dirs, events

    def _log(self, name, args, kw):
        self.events.append((name, plain(args), plain(kw)))

    def _ranked(self, count, which=False, device=False):
        out = [page(count, ROWS, np.int32), page(count, SCORES, np.float32, 0), np.array([3], np.int64), page(count, [1, 0, 1], np.int32) if which else None]
        return tuple(torch.from_numpy(a) if device and a is not None else a for a in out)

    def rank(self, *a, **kw):
        self._log("rank", a, kw)
        return self._ranked(a[2])[:3]

    def rank_device(self, *a, **kw):
        self._log("rank_device", a, kw)
        return self._ranked(a[2], device=True)[:3]

    def rank_like(self, *a, **kw):
        self._log("rank_like", a, kw)
        return self._ranked(a[2])[:3]

    def rank_like_device(self, *a, **kw):
        self._log("rank_like_device", a, kw)
        return self._ranked(a[2], device=True)[:3]

    def rank_terms(self, *a, **kw):
        self._log("rank_terms", a, kw)
        return self._ranked(kw["count"], kw["which"])

    def rank_terms_device(self, *a, **kw):
        self._log("rank_terms_device", a, kw)
        return self._ranked(kw["count"], kw["which"], device=True)

    def timeline(self, *a, **kw):
        self._log("timeline", a, kw)
        return np.arange(a[3], dtype=np.int64)[None], np.array([3], np.int64)

    def timeline_terms(self, *a, **kw):
        self._log("timeline_terms", a, kw)
        return np.arange(a[2], dtype=np.int64)[None], np.array([3], np.int64)

    def rank_near(self, *a, **kw):
        self._log("rank_near", a, kw)
        return self._ranked(kw["count"])[:3] + (page(kw["count"], [4, 5, 7], np.int32), page(kw["count"], [0.5, 0.25, 0.125], np.float32, 0), 5)

    def timeline_near(self, *a, **kw):
        self._log("timeline_near", a, kw)
        return np.arange(kw["n_bins"], dtype=np.int64)[None], np.array([3], np.int64), 5

    def digest(self, *a, **kw):
        self._log("digest", a, kw)
        none = _lib.ROW_NO_TS
        return (np.array([0, 3, -1], np.int32), np.array([2, 1, 0], np.int32), np.array([100, none, 0], np.int32), np.array([110, none, 0], np.int32),
                np.array([2, 3, 1], np.int64))

    def sightings(self, *a, **kw):
        self._log("sightings", a, kw)
        n = len(a[0])
        groups = np.zeros((n, self.n_dirs), np.int64)
        groups[0, -2:] = (1, 2)
        return (np.array([3, 0][:n], np.int64), np.array([6, -1][:n], np.int64), np.array([0.9375, -np.inf][:n], np.float32), groups, 4)

    def _thinned(self, count, device):
        out = (page(count, [3, 6], np.int32), page(count, [0.875, 0.625], np.float32, 0), page(count, [1, 0], np.int32, 0), np.array([2], np.int64))
        return tuple(torch.from_numpy(a) for a in out) if device else out

    def distinct(self, *a, **kw):
        self._log("distinct", a, kw)
        return self._thinned(a[4], False)

    def distinct_device(self, *a, **kw):
        self._log("distinct_device", a, kw)
        return self._thinned(a[4], True)

    def fetch(self, *a, **kw):
        self._log("fetch", a, kw)
        return np.array([[(int(r) + 1) / 16] * DIM for r in a[0]], np.float32)

    def scores(self, *a, **kw):
        self._log("scores", a, kw)
        n_q = 1 if np.ndim(a[0]) == 1 else len(a[0])
        return np.array([[(r + 1 + i) / 16 for r in range(self.n_rows)] for i in range(n_q)], np.float32)

    def search(self, *a, **kw):
        self._log("search", a, kw)
        return page(a[1], ROWS, np.int32), page(a[1], SCORES, np.float32, 0)

    def search_tracks(self, *a, **kw):
        self._log("search_tracks", a, kw)
        return page(a[1], ROWS, np.int32), page(a[1], SCORES, np.float32, 0)


class Hiding:
    """The same index without some of its methods, as tools/dev/rank_pages.py's WithoutRank hides `rank`."""

    def __init__(self, index, hidden):
        self.dim = index.dim
        for name in METHODS:
            if name not in hidden:
                setattr(self, name, getattr(index, name))


class Model:
    def __init__(self, events):
        self.events, self.device = events, 0

    def _encode_text(self, query):
        self.events.append(("encode", query))
        return Tensor(np.full(DIM, 0.5, np.float32))


def finder(world, hidden):
    """world: "good" (the eight crops), "bad" (and the folder with the name that does not parse), "empty" (nothing stored), "new" (an
    ObjectFinder that was never initialised: argument checks need no state)."""
    events = []
    if world == "new":
        return O.ObjectFinder.__new__(O.ObjectFinder), events
    f = O.ObjectFinder(BASE)
    f.model = Model(events)
    if world != "empty":
        table = O._RowTable()
        table.extend(P + (BAD if world == "bad" else []))
        index = Recorder(len(table.paths), len(table.dirs), events)
        f._attached = True
        f._dev["store"] = (Hiding(index, hidden) if hidden else index, table)
    return f, events


W = dict(ts_range=(100, 300), classes=[0, 2])
TS = dict(ts_range=(0, 1000))                                             # hides the name that does not parse: it carries no ts
NAN = float("nan")
T3 = [O.Term(text="van"), O.Term(path=P[3], role="require", cut=0.25), O.Term(embedding=VEC, role="reject", cut=0.75)]
SHORT = np.zeros(3, np.float32)

# (id, world, hidden methods, question, positional arguments, keyword arguments)
CASES = [
    # ---- search_page
    ("page", "good", (), "search_page", ("van",), {}),
    ("page where", "good", (), "search_page", (), dict(text_embedding=VEC, start=1, count=2, min_score=0.25, **W)),
    ("page distinct", "good", (), "search_page", (), dict(text_embedding=VEC, distinct=0.875, distinct_depth=5, count=2)),
    ("page distinct where", "good", (), "search_page", ("van",), dict(distinct=0.875, start=1, min_score=0.25, **W)),
    ("page folder without track ids", "good", (), "search_page", (), dict(text_embedding=VEC, cam_name="back", timestamp="2026-01-01")),
    ("page no live folder", "good", (), "search_page", ("van",), dict(cam_name="nowhere")),
    ("page nothing stored", "empty", (), "search_page", ("van",), {}),
    ("page bad folder", "bad", (), "search_page", (), dict(text_embedding=VEC, min_score=0.5)),
    ("page bad folder hidden", "bad", (), "search_page", (), dict(text_embedding=VEC, min_score=0.5, start=1, count=3, **TS)),
    ("page bad folder hidden distinct", "bad", (), "search_page", (), dict(text_embedding=VEC, min_score=0.5, distinct=0.875, distinct_depth=3, **TS)),
    ("page bad folder hidden cannot thin", "bad", ("distinct",), "search_page", (), dict(text_embedding=VEC, distinct=0.875, **TS)),
    ("page bad folder not live", "bad", (), "search_page", (), dict(text_embedding=VEC, cam_name="front")),
    ("page without rank", "good", ("rank",), "search_page", ("van",), dict(min_score=0.75)),
    ("page wrong dimension", "good", (), "search_page", (), dict(text_embedding=SHORT)),
    ("page start", "new", (), "search_page", ("van",), dict(start=-1)),
    ("page count", "new", (), "search_page", ("van",), dict(count=0)),
    ("page nan", "new", (), "search_page", ("van",), dict(min_score=NAN)),
    ("page distinct nan", "new", (), "search_page", ("van",), dict(distinct=NAN)),
    ("page distinct depth", "new", (), "search_page", ("van",), dict(distinct=0.5, distinct_depth=0)),
    ("page ts_range", "new", (), "search_page", ("van",), dict(ts_range=(5, 4))),
    # ---- similar
    ("similar", "good", (), "similar", (P[0],), {}),
    ("similar endpoint where", "good", (), "similar", ("/front/objects/2026-01-01/100.0_1_0.jpg",), dict(start=1, count=2, min_score=0.25, exclude="rows", **W)),
    ("similar distinct", "good", (), "similar", (P[6],), dict(distinct=0.875, distinct_depth=4, count=1)),
    ("similar whole track", "good", (), "similar", (P[1],), dict(whole_track=True, exclude="track")),
    ("similar whole track no id", "good", (), "similar", (P[2],), dict(whole_track=True, exclude="track")),
    ("similar unknown", "good", (), "similar", ("nope.jpg",), {}),
    ("similar unknown and no capability", "good", ("rank_like",), "similar", ("nope.jpg",), {}),
    ("similar no capability", "good", ("rank_like",), "similar", (P[0],), {}),
    ("similar no live folder", "good", (), "similar", (P[0],), dict(cam_name="nowhere")),
    ("similar nothing stored", "empty", (), "similar", (P[0],), {}),
    ("similar bad folder", "bad", (), "similar", (P[0],), {}),
    ("similar bad folder hidden", "bad", (), "similar", (P[0],), dict(min_score=0.25, start=1, count=3, **TS)),
    ("similar bad folder hidden whole track", "bad", (), "similar", (P[1],), dict(whole_track=True, exclude="track", **TS)),
    ("similar bad folder hidden rows distinct", "bad", (), "similar", (P[3],), dict(exclude="rows", distinct=0.875, **TS)),
    ("similar start", "new", (), "similar", (P[0],), dict(start=-1)),
    ("similar nan", "new", (), "similar", (P[0],), dict(min_score=NAN)),
    ("similar exclude", "new", (), "similar", (P[0],), dict(exclude="all")),
    # ---- compound
    ("compound", "good", (), "compound", (T3,), {}),
    ("compound where sum", "good", (), "compound", ([("van",), (None, P[0], None, "rank", -0.5)],),
     dict(combine="sum", start=1, count=2, min_score=0.125, exclude="track", **W)),
    ("compound explain", "good", (), "compound", (T3,), dict(explain=True)),
    ("compound distinct", "good", (), "compound", (T3,), dict(distinct=0.875, distinct_depth=6, start=1)),
    ("compound distinct explain", "good", (), "compound", (T3,), dict(distinct=0.875, explain=True)),
    ("compound no id track", "good", (), "compound", ([O.Term(path=P[2])],), dict(exclude="track")),
    ("compound unknown", "good", (), "compound", ([O.Term(text="van"), O.Term(path="nope.jpg")],), {}),
    ("compound wrong dimension", "good", (), "compound", ([O.Term(text="van"), O.Term(embedding=SHORT)],), {}),
    ("compound no capability", "good", ("rank_terms",), "compound", ([O.Term(path="nope.jpg")],), {}),
    ("compound no live folder", "good", (), "compound", (T3,), dict(timestamp="2027-01-01")),
    ("compound nothing stored", "empty", (), "compound", (T3,), {}),
    ("compound bad folder", "bad", (), "compound", (T3,), TS),
    ("compound bad folder not live", "bad", (), "compound", (T3,), dict(cam_name="back")),
    ("compound start", "new", (), "compound", (T3,), dict(start=-1)),
    ("compound combine", "new", (), "compound", (T3,), dict(combine="mean")),
    ("compound exclude", "new", (), "compound", (T3,), dict(exclude="all")),
    ("compound nan", "new", (), "compound", (T3,), dict(min_score=NAN)),
    # ---- compound_timeline
    ("compound_timeline", "good", (), "compound_timeline", (T3,), dict(n_bins=4)),
    ("compound_timeline where", "good", (), "compound_timeline", (T3,), dict(t0=50, bin_seconds=100, n_bins=3, combine="min", min_score=0.25, **W)),
    ("compound_timeline no live folder", "good", (), "compound_timeline", (T3,), dict(cam_name="nowhere", n_bins=3)),
    ("compound_timeline nothing stored", "empty", (), "compound_timeline", (T3,), dict(n_bins=3)),
    ("compound_timeline bad folder", "bad", (), "compound_timeline", (T3,), {}),
    ("compound_timeline bins", "new", (), "compound_timeline", (T3,), dict(n_bins=4097)),
    # ---- together
    ("together", "good", (), "together", ("person", "white van"), {}),
    ("together where", "good", (), "together", (P[0], VEC),
     dict(within=10, start=1, count=2, min_score=None, min_partner=0.25, value="a", partners=2, with_classes=[2], **W)),
    ("together terms", "good", (), "together", (O.Term(embedding=VEC), O.Term(path="/back/objects/2026-01-02/400.0_4_7.jpg")), dict(with_classes=[7])),
    ("together unknown", "good", (), "together", ("person", "nope.jpg"), {}),
    ("together wrong dimension", "good", (), "together", (SHORT, "person"), {}),
    ("together no capability", "good", ("rank_near",), "together", ("person", "nope.jpg"), {}),
    ("together no live folder", "good", (), "together", ("person", P[0]), dict(cam_name="nowhere")),
    ("together nothing stored", "empty", (), "together", ("person", "white van"), {}),
    ("together bad folder", "bad", (), "together", ("person", "white van"), TS),
    ("together start", "new", (), "together", (VEC, VEC), dict(count=0)),
    ("together value", "new", (), "together", (VEC, VEC), dict(value="max")),
    ("together within", "new", (), "together", (VEC, VEC), dict(within=-1)),
    ("together partners", "new", (), "together", (VEC, VEC), dict(partners=0)),
    ("together nan", "new", (), "together", (VEC, VEC), dict(min_partner=NAN)),
    ("together side", "new", (), "together", (VEC, None), {}),
    # ---- together_timeline
    ("together_timeline", "good", (), "together_timeline", ("person", P[3]), dict(n_bins=4)),
    ("together_timeline where", "good", (), "together_timeline", (VEC, "white van"),
     dict(within=5, t0=50, bin_seconds=100, n_bins=3, value="a", partners=7, with_classes=[2], **W)),
    ("together_timeline no live folder", "good", (), "together_timeline", (VEC, VEC), dict(cam_name="nowhere", n_bins=3)),
    ("together_timeline nothing stored", "empty", (), "together_timeline", (VEC, VEC), dict(n_bins=3)),
    ("together_timeline bad folder", "bad", (), "together_timeline", (VEC, VEC), {}),
    ("together_timeline bins", "new", (), "together_timeline", (VEC, VEC), dict(bin_seconds=0)),
    # ---- search: search_tracks, rank, the candidate loop, the full score vector
    ("search tracks", "good", (), "search", ("van",), {}),
    ("search rank past 1024", "good", (), "search", (), dict(text_embedding=VEC, top_k=2000)),
    ("search rank no track ids", "good", (), "search", (), dict(text_embedding=VEC, top_k=3, cam_name="back", timestamp="2026-01-01")),
    ("search rank where", "good", (), "search", ("van",), dict(top_k=2, **W)),
    ("search loop", "good", ("rank", "search_tracks"), "search", (), dict(text_embedding=VEC, top_k=2)),
    ("search loop no track ids", "good", ("rank",), "search", (), dict(text_embedding=VEC, cam_name="back", timestamp="2026-01-01")),
    ("search full vector", "good", ("rank",), "search", (), dict(text_embedding=VEC, top_k=4, **W)),
    ("search top_k 0", "good", (), "search", ("van",), dict(top_k=0)),
    ("search no live folder", "good", (), "search", ("van",), dict(cam_name="nowhere")),
    ("search nothing stored", "empty", (), "search", ("van",), {}),
    ("search bad folder", "bad", (), "search", ("van",), {}),
    ("search bad folder hidden", "bad", (), "search", (), dict(text_embedding=VEC, top_k=4, **TS)),
    ("search wrong dimension", "good", (), "search", (), dict(text_embedding=SHORT)),
    ("search ts_range", "new", (), "search", ("van",), dict(ts_range=(5, 4))),
    # ---- timeline
    ("timeline", "good", (), "timeline", ("van",), dict(n_bins=4)),
    ("timeline where", "good", (), "timeline", (), dict(text_embedding=VEC, t0=50, bin_seconds=100, n_bins=3, min_score=None, cam_name="front", **W)),
    ("timeline no live folder", "good", (), "timeline", ("van",), dict(cam_name="nowhere", n_bins=3)),
    ("timeline nothing stored", "empty", (), "timeline", ("van",), dict(n_bins=3)),
    ("timeline bad folder", "bad", (), "timeline", ("van",), {}),
    ("timeline bad folder hidden", "bad", (), "timeline", (), dict(text_embedding=VEC, t0=50, bin_seconds=100, n_bins=4, min_score=0.25, **TS)),
    ("timeline without timeline", "good", ("timeline",), "timeline", ("van",), dict(t0=0, bin_seconds=150, n_bins=2, min_score=0.75)),
    ("timeline bins", "new", (), "timeline", ("van",), dict(n_bins=0)),
    ("timeline nan", "new", (), "timeline", ("van",), dict(min_score=NAN)),
    # ---- digest
    ("digest", "good", (), "digest", (), {}),
    ("digest where first", "good", (), "digest", (), dict(cam_name="front", same_at=0.75, start=1, count=2000, by="first", **W)),
    ("digest no live folder", "good", (), "digest", (), dict(cam_name="nowhere")),
    ("digest nothing stored", "empty", (), "digest", (), {}),
    ("digest no capability", "good", ("digest",), "digest", (), {}),
    ("digest bad folder", "bad", (), "digest", (), {}),
    ("digest bad folder hidden", "bad", (), "digest", (), TS),
    ("digest start", "new", (), "digest", (), dict(start=-1)),
    ("digest nan", "new", (), "digest", (), dict(same_at=NAN)),
    ("digest by", "new", (), "digest", (), dict(by="new")),
    # ---- seen_before
    ("seen_before all is today", "good", (), "seen_before", (), {}),
    ("seen_before", "good", (), "seen_before", (), dict(cam_name="front", timestamp="2026-01-01")),
    ("seen_before where count", "good", (), "seen_before", (),
     dict(cam_name="front", timestamp="2026-01-01", same_at=0.75, start=1, count=5, history_cam="back", by="count", **W)),
    ("seen_before first", "good", (), "seen_before", (), dict(cam_name="front", by="first", count=1)),
    ("seen_before no live folder", "good", (), "seen_before", (), dict(cam_name="nowhere")),
    ("seen_before nothing stored", "empty", (), "seen_before", (), {}),
    ("seen_before no capability", "good", ("sightings",), "seen_before", (), {}),
    ("seen_before bad folder", "bad", (), "seen_before", (), {}),
    ("seen_before bad folder hidden", "bad", (), "seen_before", (), dict(cam_name="gate", **TS)),
    ("seen_before count", "new", (), "seen_before", (), dict(count=0)),
    ("seen_before nan", "new", (), "seen_before", (), dict(same_at=NAN)),
    ("seen_before by", "new", (), "seen_before", (), dict(by="score")),
]


def run(case):
    """-> (events, ("returns", value) or ("raises", exception class name, its text))"""
    _, world, hidden, question, args, kw = case
    f, events = finder(world, hidden)
    try:
        outcome = ("returns", plain(getattr(f, question)(*args, **kw)))
    except Exception as e:                                                 # noqa: BLE001  which one and with what text is what is recorded
        outcome = ("raises", type(e).__name__, str(e))
    return events, outcome


# ---- what the parent of the change that introduced this file answered; shorthands for what repeats ---------------------------------------
Q, V = "float32[0.5, 0.5, 0.5, 0.5]", "float32[1.0, 0.0, 0.0, 0.0]"      # the encoded text, VEC
ALL, ALL_BAD = "uint8[0, 1, 1, 1, 1]", "uint8[0, 1, 1, 1, 1, 1]"          # every folder allowed: the first table, the second
FRONT, BACK_1 = "uint8[0, 1, 1, 0, 0]", "uint8[0, 0, 0, 1, 0]"
WK, TK = {"ts_range": (100, 300), "classes": [0, 2]}, {"ts_range": (0, 1000), "classes": None}
ENC = ("encode", "van")
R3 = [(P[3], 0.875), (P[0], 0.75), (P[6], 0.625)]                         # ROWS / SCORES as results
THIN = ([(P[3], 0.875, 1), (P[6], 0.625, 0)], 2)                          # what the stub's distinct keeps
NEAR3 = [(P[3], 0.875, P[4], 0.5, 100), (P[0], 0.75, P[5], 0.25, 210), (P[6], 0.625, P[7], 0.125, 10)]
BINS4, BINS3, NO_BINS3 = ("int64[0, 1, 2, 3]", 3), ("int64[0, 1, 2]", 3), ("int64[0, 0, 0]", 0)
DIGEST2 = [(P[0], 2, 100, 110), (P[3], 1, None, None)]
DIGEST_INFO = {"objects": 2, "crops": 3, "left_over": 1}
NO_DIGEST = ([], {"objects": 0, "crops": 0, "left_over": 0})
NEW = (P[3], 1, None, None, 0, 0, [], None, None, None)
SEEN = (P[0], 2, 100, 110, 3, 2, ["back"], "2026-01-02", P[6], 0.9375)
SEEN_INFO = {"objects": 2, "new": 1, "crops": 3, "left_over": 1, "history_crops": 4}
NO_SEEN = ([], {"objects": 0, "new": 0, "crops": 0, "left_over": 0, "history_crops": 0})
NO_NEAR = ([], {"total": 0, "partners": 0, "partners_left": 0})
BAD_NAME = ("raises", "ValueError", "could not convert string to float: 'bad'")
BAD_DIR = f"{BASE}/gate/objects/2026-01-01/"


def ret(value):
    return ("returns", value)


def err(kind, text):
    return ("raises", kind, text)


def walked(n):
    """the stub's ranking of depth n as `distinct_device` is handed it"""
    return "int32[[3, 0, 6" + ", -1" * (n - 3) + "]]", "float32[[0.875, 0.75, 0.625" + ", 0.0" * (n - 3) + "]]"


def ask3(**over):
    """what T3 asks of rank_terms / timeline_terms: the vectors first (terms 0 and 2), then the stored row (term 1)"""
    return {**dict(q="float32[[0.5, 0.5, 0.5, 0.5], [1.0, 0.0, 0.0, 0.0]]", rows="int64[3]", roles=["rank", "reject", "require"], weights=[1.0, 1.0, 1.0],
                   cuts=[None, 0.75, 0.25], combine="max", allowed=ALL, min_score=None, tracks=True, exclude=None), **over}


def near(**over):
    return {**dict(within=30, partners=4096, cut_b=0.21, value="min", allowed=ALL, min_score=0.21, tracks=True), **over}


EXPECTED = {
    "page": ([ENC, ("rank", (Q, 0, 8, ALL, None), {"tracks": True})], ret((R3, 3))),
    "page where": ([("rank", (V, 1, 2, ALL, 0.25), {"tracks": True, **WK})], ret((R3[:2], 3))),
    "page distinct": ([("rank_device", (V, 0, 5, ALL, None), {"tracks": True, "with_total": False}), ("distinct_device", (*walked(5), 0.875, 0, 2), {})],
                      ret(THIN)),
    "page distinct where": ([ENC, ("rank_device", (Q, 0, 8, ALL, 0.25), {"tracks": True, "with_total": False, **WK}),
                             ("distinct_device", (*walked(8), 0.875, 1, 8), {})], ret(THIN)),
    "page folder without track ids": ([("rank", (V, 0, 8, BACK_1, None), {"tracks": False})], ret((R3, 3))),
    "page no live folder": ([ENC], ret(([], 0))),
    "page nothing stored": ([], ret(([], 0))),
    "page bad folder": ([("scores", (V,), {})], BAD_NAME),
    "page bad folder hidden": ([("scores", (V,), {})], ret(([(P[7], 0.5)], 2))),
    "page bad folder hidden distinct": ([("scores", (V,), {}), ("distinct", ("int32[9, 7]", "float32[0.625, 0.5]", 0.875, 0, 2), {})], ret(THIN)),
    "page bad folder hidden cannot thin": ([("scores", (V,), {})], err("RuntimeError", "this index cannot thin its answers")),
    "page bad folder not live": ([("rank", (V, 0, 10, "uint8[0, 1, 1, 0, 0, 0]", None), {"tracks": True})], ret((R3, 3))),
    "page without rank": ([ENC, ("search_tracks", (Q, 8, ALL), {})], ret((R3[:2], 2))),
    "page wrong dimension": ([], err("ValueError", "query has 3 dimensions, the crop index 4")),
    "page start": ([], err("ValueError", "search_page needs start >= 0 and count >= 1")),
    "page count": ([], err("ValueError", "search_page needs start >= 0 and count >= 1")),
    "page nan": ([], err("ValueError", "min_score is NaN")),
    "page distinct nan": ([], err("ValueError", "distinct is NaN")),
    "page distinct depth": ([], err("ValueError", "distinct_depth must be in [1, 1024]")),
    "page ts_range": ([], err("ValueError", "ts_range (5, 4) is empty")),
    "similar": ([("rank_like", ("int64[0]", 0, 8, ALL, None), {"tracks": True, "exclude": None})], ret((R3, 3))),
    "similar endpoint where": ([("rank_like", ("int64[0]", 1, 2, ALL, 0.25), {"tracks": True, "exclude": "rows", **WK})], ret((R3[:2], 3))),
    "similar distinct": ([("rank_like_device", ("int64[6]", 0, 4, ALL, None), {"tracks": True, "exclude": None, "with_total": False}),
                          ("distinct_device", (*walked(4), 0.875, 0, 1), {})], ret(([(P[3], 0.875, 1)], 2))),
    "similar whole track": ([("rank_like", ("int64[0, 1]", 0, 8, ALL, None), {"tracks": True, "exclude": "track"})], ret((R3, 3))),
    "similar whole track no id": ([("rank_like", ("int64[2]", 0, 8, ALL, None), {"tracks": True, "exclude": "rows"})], ret((R3, 3))),
    "similar unknown": ([], err("KeyError", "'nope.jpg'")),
    "similar unknown and no capability": ([], err("KeyError", "'nope.jpg'")),
    "similar no capability": ([], err("RuntimeError", "this index cannot be queried by its stored rows")),
    "similar no live folder": ([], ret(([], 0))),
    "similar nothing stored": ([], ret(([], 0))),
    "similar bad folder": ([("fetch", ("int64[0]",), {}), ("scores", ("float32[0.0625, 0.0625, 0.0625, 0.0625]",), {})], BAD_NAME),
    "similar bad folder hidden": ([("fetch", ("int64[0]",), {}), ("scores", ("float32[0.0625, 0.0625, 0.0625, 0.0625]",), {})],
                                  ret(([(P[7], 0.5), (P[5], 0.375), (P[3], 0.25)], 4))),
    "similar bad folder hidden whole track": ([("fetch", ("int64[0, 1]",), {}), ("scores", ("float32[0.125, 0.125, 0.125, 0.125]",), {}),
                                               ("scores", ("float32[[0.0625, 0.0625, 0.0625, 0.0625], [0.125, 0.125, 0.125, 0.125]]",), {})],
                                              ret(([(BAD[1], 0.6875), (P[7], 0.5625), (P[5], 0.4375), (P[3], 0.3125)], 4))),
    "similar bad folder hidden rows distinct": ([("fetch", ("int64[3]",), {}), ("scores", ("float32[0.25, 0.25, 0.25, 0.25]",), {}),
                                                 ("scores", ("float32[[0.25, 0.25, 0.25, 0.25]]",), {}),
                                                 ("distinct", ("int32[9, 7, 5, 1]", "float32[0.625, 0.5, 0.375, 0.125]", 0.875, 0, 4), {})], ret(THIN)),
    "similar start": ([], err("ValueError", "similar needs start >= 0 and count >= 1")),
    "similar nan": ([], err("ValueError", "min_score is NaN")),
    "similar exclude": ([], err("ValueError", 'exclude: None, "rows" or "track"')),
    "compound": ([ENC, ("rank_terms", (), ask3(start=0, count=8, which=False))], ret((R3, 3))),
    "compound where sum": ([ENC, ("rank_terms", (), ask3(start=1, count=2, which=False, q="float32[[0.5, 0.5, 0.5, 0.5]]", rows="int64[0]", roles=["rank", "rank"],
                                                         weights=[1.0, -0.5], cuts=[None, None], combine="sum", min_score=0.125, exclude="track", **WK))],
                           ret((R3[:2], 3))),
    "compound explain": ([ENC, ("rank_terms", (), ask3(start=0, count=8, which=True))], ret(([R3[0] + (2,), R3[1] + (0,), R3[2] + (2,)], 3))),
    "compound distinct": ([ENC, ("rank_terms_device", (), ask3(start=0, count=6, with_total=False, which=False)),
                           ("distinct_device", (*walked(6), 0.875, 1, 6), {})], ret(THIN)),
    "compound distinct explain": ([ENC, ("rank_terms_device", (), ask3(start=0, count=8, with_total=False, which=True)),
                                   ("distinct_device", (*walked(8), 0.875, 0, 8), {})], ret(([(P[3], 0.875, 1, 2), (P[6], 0.625, 0, 2)], 2))),
    "compound no id track": ([("rank_terms", (), ask3(start=0, count=8, which=False, q=None, rows="int64[2]", roles=["rank"], weights=[1.0], cuts=[None],
                                                      exclude="rows"))], ret((R3, 3))),
    "compound unknown": ([], err("KeyError", "'nope.jpg'")),
    "compound wrong dimension": ([], err("ValueError", "a Term's embedding has 3 dimensions, the crop index 4")),
    "compound no capability": ([], err("RuntimeError", "this index cannot rank compound questions")),
    "compound no live folder": ([], ret(([], 0))),
    "compound nothing stored": ([], ret(([], 0))),
    "compound bad folder": ([], err("ValueError", f"compound search cannot rank the folder {BAD_DIR}: it holds crop names that do not parse")),
    "compound bad folder not live": ([ENC, ("rank_terms", (), ask3(start=0, count=10, which=False, allowed="uint8[0, 0, 0, 1, 1, 0]"))], ret((R3, 3))),
    "compound start": ([], err("ValueError", "compound needs start >= 0 and count >= 1")),
    "compound combine": ([], err("ValueError", 'combine: "max", "min" or "sum"')),
    "compound exclude": ([], err("ValueError", 'exclude: None, "rows" or "track"')),
    "compound nan": ([], err("ValueError", "min_score is NaN")),
    "compound_timeline": ([ENC, ("timeline_terms", (0, 3600, 4), ask3())], ret(BINS4)),
    "compound_timeline where": ([ENC, ("timeline_terms", (50, 100, 3), ask3(combine="min", min_score=0.25, **WK))], ret(BINS3)),
    "compound_timeline no live folder": ([], ret(NO_BINS3)),
    "compound_timeline nothing stored": ([], ret(NO_BINS3)),
    "compound_timeline bad folder": ([], err("ValueError", f"compound search cannot rank the folder {BAD_DIR}: it holds crop names that do not parse")),
    "compound_timeline bins": ([], err("ValueError", "compound_timeline needs bin_seconds >= 1 and 1 <= n_bins <= 4096")),
    "together": ([("encode", "person"), ("encode", "white van"), ("rank_near", (), near(start=0, count=8, a=Q, b=Q))],
                 ret((NEAR3, {"total": 3, "partners": 5, "partners_left": 0}))),
    "together where": ([("rank_near", (), near(start=1, count=2, a=0, b=V, within=10, partners=2, cut_b=0.25, value="a", min_score=None, b_classes=[2], **WK))],
                       ret((NEAR3[:2], {"total": 3, "partners": 2, "partners_left": 3}))),
    "together terms": ([("rank_near", (), near(start=0, count=8, a=V, b=6, b_classes=[7]))], ret((NEAR3, {"total": 3, "partners": 5, "partners_left": 0}))),
    "together unknown": ([("encode", "person")], err("KeyError", "'nope.jpg'")),
    "together wrong dimension": ([], err("ValueError", "a side of together has 3 dimensions, the crop index 4")),
    "together no capability": ([], err("RuntimeError", "this index cannot join two questions")),
    "together no live folder": ([("encode", "person")], ret(NO_NEAR)),
    "together nothing stored": ([], ret(NO_NEAR)),
    "together bad folder": ([("encode", "person"), ("encode", "white van")],
                            err("ValueError", f"together cannot rank the folder {BAD_DIR}: it holds crop names that do not parse")),
    "together start": ([], err("ValueError", "together needs start >= 0 and count >= 1")),
    "together value": ([], err("ValueError", 'value: "a" or "min"')),
    "together within": ([], err("ValueError", "within: seconds in [0, 2^31)")),
    "together partners": ([], err("ValueError", "partners must be in [1, 16384]")),
    "together nan": ([], err("ValueError", "min_score / min_partner is NaN")),
    "together side": ([], err("ValueError", "a side of together needs exactly one of text, path and embedding")),
    "together_timeline": ([("encode", "person"), ("timeline_near", (), near(t0=0, bin_seconds=3600, n_bins=4, a=Q, b=3))], ret(BINS4)),
    "together_timeline where": ([("encode", "white van"), ("timeline_near", (), near(t0=50, bin_seconds=100, n_bins=3, a=V, b=Q, within=5, partners=7, value="a",
                                                                                    b_classes=[2], **WK))], ret(BINS3)),
    "together_timeline no live folder": ([], ret(NO_BINS3)),
    "together_timeline nothing stored": ([], ret(NO_BINS3)),
    "together_timeline bad folder": ([], err("ValueError", f"together cannot rank the folder {BAD_DIR}: it holds crop names that do not parse")),
    "together_timeline bins": ([], err("ValueError", "together_timeline needs bin_seconds >= 1 and 1 <= n_bins <= 4096")),
    "search tracks": ([ENC, ("search_tracks", (Q, 10, ALL), {})], ret(R3)),
    "search rank past 1024": ([("rank", (V, 0, 8, ALL, None), {"tracks": True})], ret(R3)),
    "search rank no track ids": ([("rank", (V, 0, 3, BACK_1, None), {"tracks": False})], ret(R3)),
    "search rank where": ([ENC, ("rank", (Q, 0, 2, ALL, None), {"tracks": True, **WK})], ret(R3[:2])),
    "search loop": ([("search", (V, 128, ALL), {})], ret(R3[:2])),
    "search loop no track ids": ([("search", (V, 160, BACK_1), {})], ret(R3)),
    "search full vector": ([("scores", (V,), {})], ret([(P[4], 0.3125), (P[3], 0.25), (P[1], 0.125)])),
    "search top_k 0": ([ENC], ret([])),
    "search no live folder": ([ENC], ret([])),
    "search nothing stored": ([], ret([])),
    "search bad folder": ([ENC, ("scores", (Q,), {})], BAD_NAME),
    "search bad folder hidden": ([("scores", (V,), {})], ret([(BAD[1], 0.625), (P[7], 0.5), (P[5], 0.375), (P[3], 0.25)])),
    "search wrong dimension": ([], err("ValueError", "query has 3 dimensions, the crop index 4")),
    "search ts_range": ([], err("ValueError", "ts_range (5, 4) is empty")),
    "timeline": ([ENC, ("timeline", (Q, 0, 3600, 4, ALL, 0.21), {"tracks": True})], ret(BINS4)),
    "timeline where": ([("timeline", (V, 50, 100, 3, FRONT, None), {"tracks": True, **WK})], ret(BINS3)),
    "timeline no live folder": ([ENC], ret(NO_BINS3)),
    "timeline nothing stored": ([], ret(NO_BINS3)),
    "timeline bad folder": ([ENC, ("scores", (Q,), {})], BAD_NAME),
    "timeline bad folder hidden": ([("scores", (V,), {})], ret(("int64[0, 1, 1, 1]", 4))),
    "timeline without timeline": ([ENC, ("search_tracks", (Q, 8, ALL), {})], ret(("int64[1, 1]", 2))),
    "timeline bins": ([], err("ValueError", "timeline needs bin_seconds >= 1 and 1 <= n_bins <= 4096")),
    "timeline nan": ([], err("ValueError", "min_score is NaN")),
    "digest": ([("digest", (0.9, 0, 100, ALL), {"by": "count"})], ret((DIGEST2, DIGEST_INFO))),
    "digest where first": ([("digest", (0.75, 1, 1024, FRONT), {"by": "first", **WK})], ret((DIGEST2, DIGEST_INFO))),
    "digest no live folder": ([], ret(NO_DIGEST)),
    "digest nothing stored": ([], ret(NO_DIGEST)),
    "digest no capability": ([], err("RuntimeError", "this index cannot summarise its rows")),
    "digest bad folder": ([], BAD_NAME),
    "digest bad folder hidden": ([("digest", (0.9, 0, 100, ALL_BAD), {"by": "count", **TK})], ret((DIGEST2, DIGEST_INFO))),
    "digest start": ([], err("ValueError", "digest needs start >= 0 and count >= 1")),
    "digest nan": ([], err("ValueError", "same_at is NaN")),
    "digest by": ([], err("ValueError", 'by: "count" or "first"')),
    "seen_before all is today": ([("digest", (0.9, 0, 1024, ALL), {"by": "first"})],
                                 ret(([SEEN[:4] + NEW[4:], NEW], {"objects": 2, "new": 2, "crops": 3, "left_over": 1, "history_crops": 0}))),
    "seen_before": ([("digest", (0.9, 0, 1024, "uint8[0, 1, 0, 0, 0]"), {"by": "first"}),
                     ("sightings", ([0, 3], 0.9, "uint8[0, 0, 1, 1, 1]"), {"classes": None, "group_counts": 5})], ret(([NEW, SEEN], SEEN_INFO))),
    "seen_before where count": ([("digest", (0.75, 0, 1024, "uint8[0, 1, 0, 0, 0]"), {"by": "first", **WK}),
                                 ("sightings", ([0, 3], 0.75, "uint8[0, 0, 0, 1, 1]"), {"classes": [0, 2], "group_counts": 5})], ret(([NEW], SEEN_INFO))),
    "seen_before first": ([("digest", (0.9, 0, 1024, FRONT), {"by": "first"}),
                           ("sightings", ([0, 3], 0.9, "uint8[0, 0, 0, 1, 1]"), {"classes": None, "group_counts": 5})], ret(([SEEN], SEEN_INFO))),
    "seen_before no live folder": ([], ret(NO_SEEN)),
    "seen_before nothing stored": ([], ret(NO_SEEN)),
    "seen_before no capability": ([], err("RuntimeError", "this index cannot summarise its rows")),
    "seen_before bad folder": ([], BAD_NAME),
    "seen_before bad folder hidden": ([("digest", (0.9, 0, 1024, "uint8[0, 0, 0, 0, 0, 1]"), {"by": "first", **TK}),
                                       ("sightings", ([0, 3], 0.9, "uint8[0, 1, 1, 1, 1, 0]"), {"classes": None, "group_counts": 6})],
                                      ret(([NEW, SEEN[:6] + (["back", "gate"],) + SEEN[7:]], SEEN_INFO))),
    "seen_before count": ([], err("ValueError", "seen_before needs start >= 0 and count >= 1")),
    "seen_before nan": ([], err("ValueError", "same_at is NaN")),
    "seen_before by": ([], err("ValueError", 'by: "new", "count" or "first"')),
}

PAGE = "start=0, count=100"
FOLDERS = "cam_name=None, timestamp=None"
BINS = "t0=0, bin_seconds=3600, n_bins=24"
FILTER = "ts_range=None, classes=None"
DISTINCT = "distinct=None, distinct_depth=1024"
NEAR_TAIL = f"{FOLDERS}, is_face=False, min_score=0.21, min_partner=0.21, value='min', {FILTER}, with_classes=None, partners=4096)"
SIGNATURES = {
    "search": f"(self, query=None, top_k=10, {FOLDERS}, text_embedding=None, is_face=False, {FILTER})",
    "search_page": f"(self, query=None, {PAGE}, {FOLDERS}, text_embedding=None, is_face=False, min_score=None, {FILTER}, {DISTINCT})",
    "timeline": f"(self, query=None, {BINS}, {FOLDERS}, text_embedding=None, is_face=False, min_score=0.21, {FILTER})",
    "similar": f"(self, path, {PAGE}, {FOLDERS}, is_face=False, min_score=None, {FILTER}, whole_track=False, exclude=None, {DISTINCT})",
    "compound": f"(self, terms, {PAGE}, combine='max', {FOLDERS}, is_face=False, min_score=None, {FILTER}, exclude=None, explain=False, {DISTINCT})",
    "compound_timeline": f"(self, terms, {BINS}, combine='max', {FOLDERS}, is_face=False, min_score=None, {FILTER}, exclude=None)",
    "together": f"(self, a, b, within=30, {PAGE}, {NEAR_TAIL}",
    "together_timeline": f"(self, a, b, within=30, {BINS}, {NEAR_TAIL}",
    "digest": f"(self, {FOLDERS}, is_face=False, same_at=0.9, {PAGE}, {FILTER}, by='count')",
    "seen_before": f"(self, {FOLDERS}, is_face=False, same_at=0.9, {PAGE}, {FILTER}, history_cam=None, by='new')",
}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_question_asks_the_index_what_it_asked_before(case, capsys):
    events, outcome = run(case)
    want_events, want_outcome = EXPECTED[case[0]]
    assert events == want_events
    assert outcome == want_outcome
    assert capsys.readouterr().out == ("No embeddings available.\n" if case[1] == "empty" else "")
    if case[1] in ("empty", "new"):
        assert events == []                                                # nothing stored, or a bad argument: no model, no index


def test_the_table_covers_every_question_and_every_index_method():
    assert sorted(EXPECTED) == sorted(c[0] for c in CASES) and len(EXPECTED) == len(CASES)
    assert {c[3] for c in CASES} == set(SIGNATURES)
    called = {e[0] for events, _ in EXPECTED.values() for e in events}
    assert called == set(METHODS) | {"encode"}
    for question in SIGNATURES:                                            # each question: an answer, nothing stored, no live folder, a bad argument
        mine = [c for c in CASES if c[3] == question]
        assert {"good", "bad", "empty", "new"} <= {c[1] for c in mine}, question
        assert any(EXPECTED[c[0]][1][0] == "returns" and EXPECTED[c[0]][0] for c in mine), question


def test_every_question_keeps_its_signature():
    for name, want in SIGNATURES.items():
        assert str(inspect.signature(getattr(O.ObjectFinder, name))) == want, name
    assert O.Term._fields == ("text", "path", "embedding", "role", "weight", "cut")
    assert O.Term._field_defaults == {"text": None, "path": None, "embedding": None, "role": "rank", "weight": 1.0, "cut": None}


def test_objects_re_exports_the_same_objects():
    """bench.py, tools/ and the tests import these names from clearcam_amd.objects, wherever they are defined."""
    import clearcam_amd.alerts
    import clearcam_amd.index
    for name in ("event_img_info", "pick_track_rows", "_RowTable", "Term", "OpenCLIP"):
        obj = getattr(O, name)
        assert obj.__module__ in ("clearcam_amd.objects", "clearcam_amd.row_table"), name
        assert getattr(sys.modules[obj.__module__], name) is obj, name
    assert O.EmbeddingIndex is clearcam_amd.index.EmbeddingIndex and O.row_filter is clearcam_amd.index.row_filter
    assert O.WatchList is clearcam_amd.alerts.WatchList and O.AlertBook is clearcam_amd.alerts.AlertBook
    from clearcam_amd.objects import (AlertBook, EmbeddingIndex, OpenCLIP, Term, WatchList, _RowTable, event_img_info,  # noqa: F401
                                      pick_track_rows, row_filter)
    assert _RowTable is O._RowTable and event_img_info is O.event_img_info and pick_track_rows is O.pick_track_rows


if __name__ == "__main__":                                                 # prints what the tables above hold, for the tree it is run on
    import pprint
    print("EXPECTED = " + pprint.pformat({c[0]: run(c) for c in CASES}, width=150, sort_dicts=False))
    print("SIGNATURES = " + pprint.pformat({q: str(inspect.signature(getattr(O.ObjectFinder, q))) for q in dict.fromkeys(c[3] for c in CASES)}, width=150))
