"""CPU checks of tests/postprocess_cases.py: the float64 references agree with the oracle, `postprocess_rows` is the oracle's old path,
and every crafted case still meets the conditions its GPU test relies on (so that a case cannot silently stop exercising its edge)."""
import numpy as np
import pytest
import torch

import postprocess_cases as pc
from clearcam_amd.weights import blazeface_anchors
from oracle import yolov9_oracle as yo


# ---- references ------------------------------------------------------------------------------------------------------------------
def test_float64_decode_agrees_with_oracle(sd_t):
    o = yo.YOLOv9Oracle("t", 640, sd_t)
    rng = np.random.default_rng(5)
    raws = [np.concatenate((rng.normal(0, 3, (2, h, w, 64)), rng.normal(-4.2, 1.2, (2, h, w, 80))), -1).astype(np.float32) for h, w in ((9, 14), (5, 7), (3, 4))]
    with torch.no_grad():
        ref = yo.decoded_rows(o.decode([torch.from_numpy(r).permute(0, 3, 1, 2) for r in raws]))
    d = pc.decode_np(raws, o.sd[o.head + "dfl.conv.weight"].numpy().reshape(16))
    got = pc.rows_of(d)
    clear = (d.gap >= 1e-6) & (np.abs(d.score - pc.CONF) > 1e-6)
    assert clear.mean() > 0.99 and 0.1 < (got[..., 4] > 0).mean() < 0.9
    assert np.abs(ref[..., :4] - got[..., :4]).max() <= 2e-3
    assert np.abs(ref[..., 4] - got[..., 4])[clear].max() <= 1e-6
    assert np.array_equal(ref[..., 5][clear], got[..., 5][clear])


def _nms_loop(rows: np.ndarray, iou_thr=np.float32(0.45)) -> np.ndarray:
    """postprocess :449-458 one row at a time in float32: stable top-300, row j dropped by ANY earlier row of its class."""
    out = np.zeros((len(rows), 300, 6), np.float32)
    for b, r in enumerate(rows):
        s = r[np.argsort(-r[:, 4], kind="stable")[:300]]
        area = (s[:, 2] - s[:, 0]) * (s[:, 3] - s[:, 1])
        for j in range(len(s)):
            iw = np.maximum(np.minimum(s[:j, 2], s[j, 2]) - np.maximum(s[:j, 0], s[j, 0]), np.float32(0))
            ih = np.maximum(np.minimum(s[:j, 3], s[j, 3]) - np.maximum(s[:j, 1], s[j, 1]), np.float32(0))
            with np.errstate(invalid="ignore", divide="ignore"):
                iou = iw * ih / (area[:j] + area[j] - iw * ih)
            if not ((iou > iou_thr) & (s[:j, 5] == s[j, 5])).any():
                out[b, j] = s[j]
    return out


def test_postprocess_rows_is_the_old_path():
    g = torch.Generator().manual_seed(3)
    y = torch.cat((torch.rand(2, 2, 700, generator=g) * 600, torch.rand(2, 2, 700, generator=g) * 80 + 1), 1)
    y = torch.cat((y, torch.rand(2, 80, 700, generator=g) * 0.4), 1).transpose(1, 2).contiguous().transpose(1, 2)       # (B,84,A)
    old = yo.YOLOv9Oracle.postprocess(y)
    rows = torch.from_numpy(yo.decoded_rows(y))
    new = yo.YOLOv9Oracle.postprocess_rows(rows)
    assert torch.equal(old, new) and 50 < int((new[..., 4] > 0).sum()) < 600 and int((old[..., 4] == 0).sum()) > 0
    assert np.array_equal(new.numpy(), _nms_loop(rows.numpy()))
    for name, (_, r) in pc.nms_launches().items():                            # and on the crafted rows, A < 300 included (zero-row padding)
        assert np.array_equal(yo.YOLOv9Oracle.postprocess_rows(torch.from_numpy(r)).numpy(), _nms_loop(r)), name


# ---- decode_kernel case ----------------------------------------------------------------------------------------------------------
def test_decode_case_conditions():
    c = pc.decode_case()
    assert [r.shape for r in c.raws] == [(3, 12, 20, 144), (3, 6, 10, 144), (3, 3, 5, 144)]
    d = pc.decode_np(c.raws, c.dfl_w)
    A = d.score.shape[1]
    assert A == 315 and 3 * A == 945 and (3 * A) % 256 != 0
    frac = (d.score >= pc.CONF).mean()
    assert 1 / 3 <= frac <= 2 / 3, frac
    assert not ((d.gap > 0) & (d.gap < 1e-6)).any() and not (np.abs(d.score - pc.CONF) <= 1e-6).any()      # the cap on near-ties: none
    assert c.dfl_w.min() >= 0 and c.dfl_w.max() <= 15 and not np.array_equal(c.dfl_w, np.arange(16))
    off = pc.level_offsets(pc.DECODE_LEVELS)
    assert {a for _, a in c.planted.values()} == {off[0], off[1] - 1, off[1], off[2] - 1, off[2], off[3] - 1}     # every level's first and last cell
    for name, (b, a) in c.planted.items():
        assert d.score[b, a] >= pc.CONF, name
    w = c.dfl_w.astype(np.float64)
    lvl = lambda a: max(l for l in range(3) if a >= off[l])                                                      # noqa: E731

    def side_dist(name, side):                                                # the DFL expectation of one side, recovered from the box
        b, a = c.planted[name]
        l = lvl(a); W = pc.DECODE_LEVELS[l][1]; s = pc.STRIDES[l]
        ax, ay = (a - off[l]) % W + 0.5, (a - off[l]) // W + 0.5
        return [ax - d.box[b, a, 0] / s, ay - d.box[b, a, 1] / s, d.box[b, a, 2] / s - ax, d.box[b, a, 3] / s - ay][side]
    assert abs(side_dist("uniform_side", 1) - w.mean()) < 1e-12 and abs(side_dist("uniform_side_l1", 1) - w.mean()) < 1e-12
    assert abs(side_dist("saturated_side", 2) - w[11]) < 1e-12 and abs(side_dist("saturated_side_l2", 2) - w[11]) < 1e-12
    assert abs(side_dist("inverse_saturated_side", 0) - (w.sum() - w[5]) / 15) < 1e-12
    for name, pair in zip(("tie_7_42", "tie_0_79", "tie_3_4"), pc.TIE_CLASSES):
        b, a = c.planted[name]
        assert d.gap[b, a] == 0 and d.cls[b, a] == pair[0] and pair[0] // 4 != pair[1] // 4, name        # different float4 groups of the scan


# ---- head_tail_kernel cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [False, True], ids=["main", "small"])
@pytest.mark.parametrize("ch", [128, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f16s"])
def test_tail_case_conditions(lib_path, dtype, ch, small):
    c = pc.tail_case(dtype, ch, small)
    M = [c.B * h * w for h, w in c.levels]
    if not small:
        assert M == [720, 180, 45] and M[0] > 512 and (M[0] - 512) % 64 == 16 and M[2] % 16 == 13       # ragged tile, ragged fragment, two blocks on level 0
    t = pc.TORCH_DT[dtype]
    for x in c.bx + c.cl:
        assert np.array_equal(x, torch.from_numpy(x).to(t).float().numpy())                             # the storage type holds the activations
    lo, hi = pc.TIE_PAIR
    assert lo // 16 != hi // 16 and (lo % 16) // 4 != (hi % 16) // 4                                    # different fragments, different lane groups
    for l in range(3):
        w3 = pc.kernel_weights(dtype, c.w3[l])
        assert np.array_equal(w3[lo], w3[hi]) and c.b3[l][lo] == c.b3[l][hi]                             # still identical after the kernel's rounding
        if dtype != "f16s":
            assert not np.array_equal(w3, c.w3[l])                                                       # the entry is handed unrounded weights
    logits = pc.tail_logits(c, dtype)
    sd = np.concatenate([x.reshape(-1, 144) for x in logits]).std(0)
    assert 1.2 < np.median(sd) < 2.8, np.median(sd)
    d = pc.decode_np(logits, c.dfl_w)
    tie = d.gap == 0
    assert (d.cls[tie] == lo).all()
    if not small:
        assert 0.02 < tie.mean() < 0.6, tie.mean()                                                      # the tied pair is the maximum on a known share
    assert tie.sum() >= 1
    assert ((d.gap > 0) & (d.gap < 1e-4)).mean() <= 0.01                                                # at most 1 % of the anchors excluded
    assert not (np.abs(d.score - pc.CONF) <= 1e-5).any()


# ---- topk_nms_kernel cases -------------------------------------------------------------------------------------------------------
def test_nms_case_conditions():
    L = pc.nms_launches()
    names, rows = L["a2100"]
    assert rows.shape[1:] == (2100, 6) and rows.dtype == np.float32
    by = dict(zip(names, rows))
    for n in (0, 1, 299, 300, 301, 511, 512, 513, 2100):
        s = by[f"nz{n}"][:, 4]
        assert (s > 0).sum() == n and len(np.unique(s[s > 0])) == n
    for name, (_, r) in L.items():
        s = r[..., 4]
        assert ((s == 0) | ((s >= 0.25) & (s <= 1))).all(), name
        assert np.array_equal(r[..., :4], np.round(r[..., :4])) and np.abs(r[..., :4]).max() < 1024, name   # integer boxes: exact areas and unions
    assert [n for n in L["a189"][0]] == ["nz0", "nz1", "nz100", "nz189", "all_equal"] and L["a189"][1].shape[1] == 189
    assert (L["a525"][1][..., 4] > 0).sum(1).tolist() == [0, 299, 300, 301, 512, 525, 525]
    post = lambda r: yo.YOLOv9Oracle.postprocess_rows(torch.from_numpy(r[None]))[0].numpy()              # noqa: E731
    # all equal: the selection is decided by the anchor index alone
    r = by["all_equal"]; srt = r[:300].copy()
    k = post(r)
    alive = k[:, 4] > 0
    assert np.array_equal(k[alive], srt[alive]) and alive.sum() > 50
    # seven values: the 300th place falls inside a run
    s = np.sort(by["seven_values"][:, 4])[::-1]
    assert (s > 0).sum() == 700 and s[299] == s[298] == s[300]
    s = by["low_byte"][:, 4]; bits = s[s > 0].view(np.uint32)
    assert len(bits) == 600 and len(np.unique(bits >> 8)) == 1 and len(np.unique(bits)) > 200
    assert (by["head200"][:200, 4] > 0).all() and (by["head200"][200:, 4] == 0).all()
    assert np.array_equal(post(by["head200"])[200:, :4] * 0, np.zeros((100, 4))) and (post(by["head200"])[200:, 4] == 0).all()
    assert (by["tail40"][:-40, 4] == 0).all() and (by["tail40"][-40:, 4] > 0).all()
    # the NMS scenarios, through the oracle
    k = post(by["pairs"])
    sc = {round(float(v), 2) for v in k[:, 4] if v > 0}
    assert sc == {0.99, 0.96, 0.95, 0.94, 0.92, 0.91, 0.90, 0.89, 0.88, 0.87, 0.86, 0.85}                # 0.98, 0.97 (chain) and 0.93 (IoU 1/2) dropped
    r = by["pairs"]
    iou = lambda a, b: (max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1]))) / \
        ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1])))   # noqa: E731
    assert iou(r[10], r[20]) <= 0.45 < iou(r[700], r[20]) and iou(r[10], r[700]) > 0.45                  # row 2 falls to the suppressed row 1 only
    assert np.float32(9) / np.float32(20) == np.float32(0.45) and iou(r[30], r[31]) == 9 / 20 and iou(r[40], r[41]) == 0.5
    g = pc.geometry(pc.UNIFORM_SRC)
    assert g[1] != 0 and g[2] != 1                                                                         # non-zero pad, gain other than 1
    e = pc.nms_expected(by["pairs"][None], [pc.UNIFORM_SRC])[0]
    assert (e[:, 0] == 0).any() and (e[:, 2] == 480).any() and (e[:, 1] == 0).any() and (e[:, 3] == 270).any()   # clipped at every edge
    k = post(by["identical300"])
    assert (k[:, 4] > 0).sum() == 1 and k[0, 4] == 1.0
    for i in (297, 298, 296):
        k = post(by[f"trio{i % 3}"])
        assert (k[:299, 4] > 0).all() and k[299, 4] == 0
    assert len({pc.geometry(s).tobytes() for s in pc.RAGGED_SRCS}) == len(pc.RAGGED_SRCS)


# ---- blaze_post_kernel cases -----------------------------------------------------------------------------------------------------
def test_blaze_case_conditions():
    anchors = blazeface_anchors()
    L = pc.blaze_launches(anchors)
    rows, first, idx = pc.blaze_expected(anchors, L["plain"])
    assert idx[0] == -1 and not first.any() and not rows.any()                                            # nothing alive, nothing moved
    P = L["padded"]
    assert P.pad_top > 0 and len(P.names) == 6
    rows, first, idx = pc.blaze_expected(anchors, P)
    by = {n: i for i, n in enumerate(P.names)}
    i = by["none_alive_padded"]
    assert idx[i] == 0 and (rows[i][:, 16] == 0).all() and first[i][0] == np.float32(-P.pad_top) / np.float32(P.scale)
    i = by["all_score_one"]
    assert np.float32(torch.sigmoid(torch.tensor(100.0))) == 1.0
    alive = rows[i][:, 16] != 0
    assert alive.sum() > 20 and (rows[i][alive, 16] == np.float32(256) / np.float32(P.scale)).all()
    # integer raws over the anchors: every decoded coordinate is a multiple of 1/512 well inside float32
    for n in ("none_alive_padded", "all_score_one", "overlap_rule", "ymin_zero"):
        r = P.raw[by[n]]
        assert np.array_equal(r * 2, np.round(r * 2)), n
    i = by["overlap_rule"]; m = pc.BLAZE_MARKS["overlap_rule"]
    alive_scores = np.sort(rows[i][rows[i][:, 16] != 0, 16].astype(np.float64) * P.scale / 256)
    kept = np.sort(torch.sigmoid(torch.from_numpy(P.score[i][[m[k] for k in ("eq_a", "eq_b", "gt_a", "ch_a")]])).numpy())
    assert len(alive_scores) == 4 and np.allclose(alive_scores, kept, atol=1e-6, rtol=0)                    # 3/10 kept; above it dropped; the chain's b and c dropped
    assert np.float32(60) / np.float32(200) == np.float32(0.3)
    i = by["ymin_zero"]; m = pc.BLAZE_MARKS["ymin_zero"]
    assert rows[i][0, 0] == 0 and rows[i][0, 16] != 0 and idx[i] == 1 and rows[i][1, 16] != 0
    for n in ("random0", "random1"):
        i = by[n]
        ds, di = pc.blaze_margins(anchors, P.raw[i], P.score[i])
        assert ds > 1e-5 and di > 1e-5, (n, ds, di)
        alive = (rows[i][:, 16] != 0).sum()
        n_over = (torch.sigmoid(torch.from_numpy(P.score[i])) >= 0.85).sum()
        assert 20 < alive < n_over                                                                         # the overlap rule drops some, keeps some
