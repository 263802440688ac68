"""Numpy models and seeded worlds for the alert tests (test_watch_host.py, test_gpu_watch.py).

`resolve` is the model of what cc_watch_match returns for a given score matrix (test_watch_host.py holds it against a literal
restatement of the reference's loop, clearcam.py:1289-1307).  A world is a seeded batch of unit
embeddings, a table of unit descriptions, cameras, thresholds at the median and 15 % of the alerts disarmed."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

WORLDS = [(200, 37, 6), (255, 300, 16), (65, 9, 2)]          # (B, A, cameras)
SEEDS = [7, 8, 9]
DIM = 768


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def product64(E, D):
    """(B, A): the float64 product rounded to float32."""
    return (E.astype(np.float64) @ D.astype(np.float64).T).astype(np.float32)


def median_thresholds(S, alert_group, crop_group):
    """thr[a] = the median of S[:, a] over the crops of alert a's camera, as float32 (2.0, which no unit score reaches, for an alert
    whose camera has no crop in the batch)."""
    thr = np.full(S.shape[1], 2.0, np.float32)
    for a in range(S.shape[1]):
        col = S[crop_group == alert_group[a], a]
        if col.size:
            thr[a] = np.float32(np.median(col))
    return thr


def resolve(S, thr, alert_group, crop_group, armed):
    """The outputs of the two kernels for the score matrix S (B, A): hit bits `S > thr && same camera`, then per crop in order the
    lowest alert that hit and is still armed fires and is spent.  -> (alert int32 (B,), score float32 (B,))."""
    S = np.asarray(S, np.float32)
    B, A = S.shape
    with np.errstate(invalid="ignore"):
        hits = (S > np.asarray(thr, np.float32)[None, :]) & (np.asarray(alert_group)[None, :] == np.asarray(crop_group)[:, None])
    live = np.ones(A, bool) if armed is None else np.asarray(armed).reshape(-1) != 0
    live = live.copy()
    alert, score = np.full(B, -1, np.int32), np.zeros(B, np.float32)
    for b in range(B):
        w = hits[b] & live
        if w.any():
            a = int(np.argmax(w))
            alert[b], score[b] = a, S[b, a]
            live[a] = False
    return alert, score


class World(NamedTuple):
    E: np.ndarray                # (B, dim) unit crop embeddings
    D: np.ndarray                # (A, dim) unit descriptions
    alert_group: np.ndarray      # (A,) camera of each alert
    crop_group: np.ndarray       # (B,) camera of each crop
    armed: np.ndarray            # (A,) uint8, 15 % zero


@lru_cache(maxsize=None)
def world(B, A, cams, seed, dim=DIM) -> World:
    rng = np.random.default_rng(seed)
    alert_group = rng.integers(0, cams, A).astype(np.int32)
    crop_group = rng.integers(0, cams, B).astype(np.int32)
    armed = np.ones(A, np.uint8)
    armed[rng.permutation(A)[:int(round(0.15 * A))]] = 0
    D, E = unit_rows(rng, A, dim), unit_rows(rng, B, dim)
    for x in (E, D, alert_group, crop_group, armed):
        x.setflags(write=False)
    return World(E, D, alert_group, crop_group, armed)


def check_not_vacuous(S, thr, w: World, armed, alert):
    """The conditions under which a world exercises the rule: at least half of the armed alerts fire, at least 4 crops receive a later
    alert than their first hit (the lowest set bit of the crop's hit word) because the earlier one was spent - by a crop before it, or
    before the batch, which is what a disarmed alert is - and at least one crop fires nothing.  -> (alerts fired, such crops)."""
    armed = np.ones(S.shape[1], np.uint8) if armed is None else np.asarray(armed)
    fired = alert[alert >= 0]
    assert len(set(fired.tolist())) == fired.size                      # an alert fires once
    assert fired.size >= 0.5 * int(armed.sum()), (fired.size, int(armed.sum()))
    hits = (S > thr[None, :]) & (w.alert_group[None, :] == w.crop_group[:, None])
    first = np.where(hits.any(1), hits.argmax(1), -1)
    later = int(((alert >= 0) & (alert > first) & (first >= 0)).sum())
    assert later >= 4, later
    assert (alert < 0).any()
    return fired.size, later
