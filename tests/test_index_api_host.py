"""The public surface of `EmbeddingIndex` as callers see it: every public method's signature against a table written down when the
class moved into clearcam_amd/index.py, and the module it is importable from.  No GPU, no library call."""
import inspect

import clearcam_amd.index
import clearcam_amd.objects
from clearcam_amd.index import EmbeddingIndex

T2 = " -> 'Tuple[np.ndarray, np.ndarray]'"
T3 = " -> 'Tuple[np.ndarray, np.ndarray, np.ndarray]'"
TERMS = "q=None, rows=None, roles=None, weights=None, cuts=None, combine: 'str' = 'max'"
NEAR = "partners: 'int' = 4096, cut_b=None, value: 'str' = 'min', allowed=None, min_score=None, tracks: 'bool' = True"
B_FILTER = "ts_range=None, classes=None, b_ts_range=None, b_classes=None"
DIGEST = ("(self, same_at: 'float' = 0.9, start: 'int' = 0, count=None, allowed=None, ts_range=None, classes=None, max_leaders: 'int' = 1024, "
          "by: 'str' = 'count', owners: 'bool' = False")
SIGHTINGS = ("(self, rows, same_at: 'float' = 0.9, allowed=None, ts_range=None, classes=None, skip_self: 'bool' = False, group_counts: 'int' = 0, "
             "with_total: 'bool' = True)")

SIGNATURES = {
    "__init__": "(self, dim: 'int' = 768, capacity: 'int' = 1048576, device: 'int' = 0, storage: 'str' = 'f32')",
    "__len__": "(self) -> 'int'",
    "add": "(self, emb, groups=None, tracks=None, ts=None, classes=None) -> 'None'",
    "close": "(self)",
    "cut_f32": "(min_score) -> 'np.float32'",
    "digest": DIGEST + ")",
    "digest_device": DIGEST + ", with_total: 'bool' = True)",
    "distinct": "(self, idx, score=None, same_at: 'float' = 0.9, start: 'int' = 0, count=None)",
    "distinct_device": "(self, idx, score=None, same_at: 'float' = 0.9, start: 'int' = 0, count=None, with_total: 'bool' = True)",
    "fetch": "(self, rows, device_out: 'bool' = False)",
    "gram": "(self, rows, device_out: 'bool' = False)",
    "last_scores_path": "(self) -> 'int'",
    "rank": "(self, q, start: 'int', count: 'int', allowed=None, min_score=None, tracks: 'bool' = True, ts_range=None, classes=None)" + T3,
    "rank_device": "(self, q, start: 'int', count: 'int', allowed=None, min_score=None, tracks: 'bool' = True, with_total: 'bool' = True, "
                   "ts_range=None, classes=None)",
    "rank_like": "(self, rows, start: 'int', count: 'int', allowed=None, min_score=None, tracks: 'bool' = True, exclude=None, ts_range=None, "
                 "classes=None)" + T3,
    "rank_like_device": "(self, rows, start: 'int', count: 'int', allowed=None, min_score=None, tracks: 'bool' = True, exclude=None, "
                        "with_total: 'bool' = True, ts_range=None, classes=None)",
    "rank_near": f"(self, a, b, within, start: 'int' = 0, count: 'int' = 100, {NEAR}, {B_FILTER})",
    "rank_near_device": f"(self, a, b, within, start: 'int' = 0, count: 'int' = 100, {NEAR}, with_total: 'bool' = True, {B_FILTER})",
    "rank_terms": f"(self, {TERMS}, start: 'int' = 0, count: 'int' = 100, allowed=None, min_score=None, tracks: 'bool' = True, exclude=None, "
                  "ts_range=None, classes=None, which: 'bool' = False)",
    "rank_terms_device": f"(self, {TERMS}, start: 'int' = 0, count: 'int' = 100, allowed=None, min_score=None, tracks: 'bool' = True, exclude=None, "
                         "with_total: 'bool' = True, ts_range=None, classes=None, which: 'bool' = False)",
    "remove": "(self, rows) -> 'int'",
    "remove_groups": "(self, drop) -> 'int'",
    "row_filter": "(ts_range=None, classes=None) -> \"Optional['_lib.RowFilter']\"",
    "row_info": "(self)" + T2,
    "scores": "(self, q) -> 'np.ndarray'",
    "search": "(self, q, k: 'int', allowed=None)" + T2,
    "search_device": "(self, q, k: 'int')",
    "search_tracks": "(self, q, k: 'int', allowed=None)" + T2,
    "search_tracks_device": "(self, q, k: 'int', allowed=None)",
    "sightings": SIGHTINGS,
    "sightings_device": SIGHTINGS,
    "timeline": "(self, q, t0: 'int', bin_seconds: 'int', n_bins: 'int', allowed=None, min_score=None, tracks: 'bool' = True, ts_range=None, "
                "classes=None)" + T2,
    "timeline_near": f"(self, a, b, within, t0: 'int', bin_seconds: 'int', n_bins: 'int', {NEAR}, {B_FILTER})",
    "timeline_terms": f"(self, t0: 'int', bin_seconds: 'int', n_bins: 'int', {TERMS}, allowed=None, min_score=None, tracks: 'bool' = True, "
                      "exclude=None, ts_range=None, classes=None)" + T2,
}


def public_methods():
    """name -> function for everything callable a user of the class can reach without an underscore (plus __init__ / __len__)"""
    out = {}
    for name, member in vars(EmbeddingIndex).items():
        if name.startswith("_") and name not in ("__init__", "__len__"):
            continue
        fn = member.__func__ if isinstance(member, (staticmethod, classmethod)) else member
        if inspect.isfunction(fn):
            out[name] = fn
    return out


def test_every_public_signature_is_the_recorded_one():
    got = {name: str(inspect.signature(fn)) for name, fn in public_methods().items()}
    assert sorted(got) == sorted(SIGNATURES)                                        # nothing gone, nothing new without a row here
    for name in SIGNATURES:
        assert got[name] == SIGNATURES[name], name


def test_the_rest_of_the_surface_stays():
    assert isinstance(vars(EmbeddingIndex)["capacity"], property)
    assert isinstance(vars(EmbeddingIndex)["cut_f32"], staticmethod) and isinstance(vars(EmbeddingIndex)["row_filter"], staticmethod)
    assert EmbeddingIndex.STORAGE == {"f32": 0, "bf16": 2, "i8": 8}
    assert set(EmbeddingIndex.LIKE_EXCLUDE) == {None, "rows", "track"} and set(EmbeddingIndex.DIGEST_BY) == {"count", "first"}
    assert set(EmbeddingIndex.TERM_ROLE) == {"rank", "require", "reject"} and set(EmbeddingIndex.COMBINE) == {"max", "min", "sum"}


def test_objects_re_exports_the_same_objects():
    assert clearcam_amd.objects.EmbeddingIndex is clearcam_amd.index.EmbeddingIndex
    assert clearcam_amd.objects.row_filter is clearcam_amd.index.row_filter
    assert EmbeddingIndex.row_filter is clearcam_amd.index.row_filter
    from clearcam_amd.objects import EmbeddingIndex as E, row_filter as f            # noqa: F401  the import callers and tools/dev use
    assert E is EmbeddingIndex and f is clearcam_amd.index.row_filter
