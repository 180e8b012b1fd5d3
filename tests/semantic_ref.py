"""float64 references of the semantic kernels (csrc/semantic.hip) in pure torch, and the crafted inputs their tests share
(tests/test_semantic_cpu.py holds the references to second statements of themselves; tests/test_semantic.py holds the
kernels to the references).  Nothing here imports the package under test.

* the K-channel forward is ``O.composite_tiles`` with the table expanded to [C,N,K] in the colour argument -- the oracle
  composites any channel count over given lists -- and the gradient of the table is its autograd;
* ``forward_by_weights`` is the second statement: per tile, ``O.blend_run``'s weights (its colour result for an identity
  colour matrix) times the rows of the table;
* ``cross_entropy`` / ``confusion`` / ``iou`` are written out by hand; the CPU test compares them with
  ``torch.nn.functional.cross_entropy`` and with hand-counted tables.
"""
from __future__ import annotations

from typing import Optional

import torch

from oracle import splat_oracle as O

TILE = 16
MARGIN = 1e-5                    # as tests/test_composite_edges.py: a decision this close to its threshold is "unsafe"
MAX_UNSAFE_SHARE = 0.005         # as tests/depth_spread_cases.py: at most 0.5 % of a case's pixels may be unsafe
CHANNELS = (1, 3, 4, 5, 8, 9, 16, 17, 32)  # 1, 3, 5, 32 and a count on each side of the kernels' chunk sizes 4, 8 and 16
IGNORE = 255


def table(n: int, k: int, seed: int = 0) -> torch.Tensor:
    """[n,k] float64 logits in about +-3, seeded."""
    g = torch.Generator().manual_seed(1000 * k + n + seed)
    return 3.0 * torch.randn(n, k, generator=g, dtype=torch.float64)


def forward(c, means2d, conics, opac, F):
    """[C,H,W,K] float64 (and the margin [C,H,W]): the table composited over the case's lists by the oracle."""
    out, _, _, margin = O.composite_tiles(means2d, conics, F[None].expand(c.C, -1, -1), opac, c.w, c.h, TILE, c.offsets,
                                          c.flatten_ids, return_margin=True)
    return out, margin


def forward_by_weights(c, means2d, conics, opac, F):
    """The same image from the blending weights themselves: per tile, w [P,K_run] = blend_run's result for an identity
    colour matrix, times the table's rows of the run's Gaussians (record cam * N + n reads row n)."""
    out = torch.zeros(c.C, c.h, c.w, F.shape[1], dtype=torch.float64)
    offs = c.offsets.reshape(-1).tolist() + [c.M]
    m2, cn, op = means2d.reshape(-1, 2), conics.reshape(-1, 3), opac.reshape(-1)
    fid = c.flatten_ids.to(torch.int64)
    ys, xs = torch.meshgrid(torch.arange(TILE), torch.arange(TILE), indexing="ij")
    T = c.tile_w * c.tile_h
    for t in range(c.C * T):
        s, e = offs[t], offs[t + 1]
        if e <= s:
            continue
        cam, ty, tx = t // T, (t % T) // c.tile_w, t % c.tile_w
        py, px = (ty * TILE + ys).reshape(-1), (tx * TILE + xs).reshape(-1)
        ins = (py < c.h) & (px < c.w)
        py, px = py[ins], px[ins]
        g = fid[s:e]
        dx = m2[g][None, :, 0] - (px.double()[:, None] + 0.5)
        dy = m2[g][None, :, 1] - (py.double()[:, None] + 0.5)
        w = O.blend_run(dx, dy, cn[g], op[g], torch.eye(e - s, dtype=torch.float64))[6]
        out[cam, py, px] = w @ F[g - cam * c.N]
    return out


def unsafe_share(margin) -> float:
    return float((~(margin > MARGIN)).double().mean())


# ---- labels -------------------------------------------------------------------------------------------------------------
LABEL_MAPS = ("mixed", "all_ignored", "absent_class", "beyond_k")


def label_map(kind: str, h: int, w: int, k: int, seed: int = 0) -> torch.Tensor:
    """uint8 [h,w].  "mixed": every class, a fifth of the pixels 255; "all_ignored": 255 everywhere; "absent_class": class 0
    never occurs (k = 1: nothing is labelled); "beyond_k": a tenth of the pixels carry k .. k + 3, which is not a class and
    not the ignore value either."""
    g = torch.Generator().manual_seed(seed + 31 * h + w + 7 * k + len(kind))
    lab = torch.randint(0, k, (h, w), generator=g)
    u = torch.rand(h, w, generator=g)
    if kind == "mixed":
        lab[u < 0.2] = IGNORE
    elif kind == "all_ignored":
        lab[:] = IGNORE
    elif kind == "absent_class":
        lab = torch.where(lab == 0, torch.full_like(lab, 1 if k > 1 else IGNORE), lab)
    elif kind == "beyond_k":
        lab = torch.where(u < 0.1, k + torch.randint(0, 4, (h, w), generator=g), lab)
        lab[(u > 0.9)] = IGNORE
    else:
        raise ValueError(kind)
    return lab.to(torch.uint8)


def logits_image(h: int, w: int, k: int, seed: int = 0, extreme: bool = True) -> torch.Tensor:
    """float32 [h,w,k]: randn logits; with ``extreme`` every seventh pixel has one channel at +80 and every eleventh one at
    -80 (log-sum-exp must be taken about the row maximum)."""
    g = torch.Generator().manual_seed(seed + 13 * h + 5 * w + k)
    x = 2.0 * torch.randn(h, w, k, generator=g)
    if extreme:
        flat = x.reshape(-1, k)
        idx = torch.arange(flat.shape[0])
        ch = torch.randint(0, k, (flat.shape[0],), generator=g)
        flat[idx[::7], ch[::7]] = 80.0
        flat[idx[::11], ch[::11]] = -80.0
    return x.float()


def class_weights(k: int) -> torch.Tensor:
    """float32 [k]: 0.5, 1.0, 1.5, ... cycled over four values."""
    return torch.tensor([0.5 + 0.5 * (i % 4) for i in range(k)], dtype=torch.float32)


def labelled(labels, k: int, ignore: int = IGNORE):
    lab = labels.reshape(-1).to(torch.int64)
    return (lab != ignore) & (lab < k)


def cross_entropy(logits, labels, ignore: int = IGNORE, weight: Optional[torch.Tensor] = None):
    """(loss, gradient [n,K]) in float64: sum_p cw[y_p] nll_p / sum_p cw[y_p] over the labelled pixels (a label >= K counts
    as ignored), 0 and zeros when the weights of the labelled pixels sum to 0."""
    k = logits.shape[-1]
    x = logits.reshape(-1, k).double()
    lab = labels.reshape(-1).to(torch.int64)
    ok = labelled(labels, k, ignore)
    y = torch.where(ok, lab, torch.zeros_like(lab))
    mx = x.amax(dim=1, keepdim=True)
    ex = torch.exp(x - mx)
    se = ex.sum(dim=1, keepdim=True)
    nll = (mx + torch.log(se))[:, 0] - x.gather(1, y[:, None])[:, 0]
    cw = torch.ones(k, dtype=torch.float64) if weight is None else weight.double()
    wp = torch.where(ok, cw[y], torch.zeros(1, dtype=torch.float64))
    total = wp.sum()
    if float(total) == 0.0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    onehot = torch.zeros_like(x).scatter_(1, y[:, None], 1.0)
    grad = wp[:, None] * (ex / se - onehot) / total
    return (wp * nll).sum() / total, grad


def confusion(logits, labels, ignore: int = IGNORE, acc=None, min_alpha: float = 0.5) -> torch.Tensor:
    """int64 [K, K + 1]: row = label, column = the first maximum of the row, or K where acc < min_alpha."""
    k = logits.shape[-1]
    x = logits.reshape(-1, k)
    lab = labels.reshape(-1).to(torch.int64)
    ok = labelled(labels, k, ignore)
    # (torch.argmax does not promise the first of equal maxima: the lowest index that equals the maximum)
    pred = torch.where(x == x.amax(dim=1, keepdim=True), torch.arange(k)[None, :], torch.full((1, 1), k)).amin(dim=1)
    if acc is not None:
        pred = torch.where(acc.reshape(-1) >= min_alpha, pred, torch.full_like(pred, k))
    out = torch.zeros(k, k + 1, dtype=torch.int64)
    out.reshape(-1).index_add_(0, lab[ok] * (k + 1) + pred[ok], torch.ones(int(ok.sum()), dtype=torch.int64))
    return out


def iou(conf: torch.Tensor):
    """(miou, pixel accuracy, per-class IoU with None for classes absent from labels and predictions) from a [K, K + 1]
    table by plain loops."""
    k = conf.shape[0]
    per = []
    for c in range(k):
        tp = int(conf[c, c])
        fn = int(conf[c].sum()) - tp
        fp = int(conf[:, c].sum()) - tp
        per.append(tp / (tp + fp + fn) if tp + fp + fn else None)
    have = [v for v in per if v is not None]
    total = int(conf.sum())
    return (sum(have) / len(have) if have else 0.0, sum(int(conf[c, c]) for c in range(k)) / total if total else 0.0, per)
