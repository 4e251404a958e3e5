"""Fixtures for per-sample mixup / CutMix (`mode='elem'` and `mode='pair'`), recorded from the reference's own code.

    python tests/golden/make_golden_mix_modes.py /path/to/reference

loads the reference's `datasets/mixup.py` and `loss/cross_entropy.py` where they lie, by file path (as make_golden_recipe.py does), runs
`FastCollateMixup(mode='elem' | 'pair')` and `SoftTargetCrossEntropy` on the CPU and writes DATA only:

  mix_modes_draws.json  for np.random.seed(SEED): 32 consecutive batches of 6 x 3 x 224 x 224 images for each mode under five settings --
                        the recipes' (mixup 0.8, cutmix 1.0, prob 1, switch 0.5), prob 0.5, cutmix_minmax [0.2, 0.8], mixup only, CutMix
                        only.  Per sample: lam as the bits of the float32 the reference keeps, use_cutmix as drawn, the box.
  mix_modes.npz         per case: the uint8 inputs and labels, the reference's mixed uint8 batch, its dense fp32 target and its lam_batch
                        (with use_cutmix and the boxes), seeded logits, and SoftTargetCrossEntropy's mean, per-row loss and gradient in
                        fp32, in fp64, and in fp64 on the bf16-rounded logits.

The cases' seeds are FOUND here, by scanning seeds upwards (at most 10 000) until the reference's first draw has the property the case is
about, so the file states the property, not a magic number.  The .npz is written with fixed zip timestamps.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_recipe import load, loss_and_grad, write_npz  # noqa: E402

SEED = 20241
RECIPE = dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, label_smoothing=0.1)
SETTINGS = {"recipe": {}, "prob_half": dict(prob=0.5), "minmax": dict(cutmix_minmax=[0.2, 0.8]), "mixup_only": dict(cutmix_alpha=0.),
            "cutmix_only": dict(mixup_alpha=0.)}
N_DRAWS, DRAW_SHAPE = 32, [6, 3, 224, 224]


def recording_collate(mx, mode, **kw):
    """FastCollateMixup(mode) whose draws are written down: after each collate `rec` holds one dict per batch -- lam (the reference's
    lam_batch after its corrections, float32 [N]), drawn (lam before them), use_cutmix (as drawn) and boxes [N, 4]"""
    rec = []
    real_bbox = mx.__dict__.setdefault("_unrecorded_bbox", mx.cutmix_bbox_and_lam)

    class Recording(mx.FastCollateMixup):
        def _params_per_elem(self, n):
            lam, use_cutmix = super()._params_per_elem(n)
            assert lam.dtype == np.float32
            rec.append(dict(lam=lam, drawn=lam.copy(), use_cutmix=np.asarray(use_cutmix, dtype=bool).copy(), calls=[]))
            return lam, use_cutmix  # (the collate stores the corrected lambdas into this very array)

    def bbox(*a, **k):
        box, lam = real_bbox(*a, **k)
        rec[-1]["calls"].append([int(v) for v in box])
        return box, lam
    mx.cutmix_bbox_and_lam = bbox
    kw = dict(RECIPE, mode=mode, **kw)
    if kw["cutmix_minmax"] is None:
        kw["cutmix_minmax"] = ()  # (the reference's constructor takes len() of it)
    return Recording(**kw), rec


def finish(r, mode):
    """one batch's record as per-sample arrays: a box belongs to each element whose drawn lam != 1 and whose switch says CutMix, in index
    order (the reference's loop); 'pair' mirrors the half it drew"""
    lam, drawn, cut = r["lam"].copy(), r["drawn"], r["use_cutmix"]
    boxes = np.zeros((len(lam), 4), dtype=np.int64)
    idx = [i for i in range(len(lam)) if drawn[i] != 1. and cut[i]]
    assert len(idx) == len(r["calls"])
    for i, b in zip(idx, r["calls"]):
        boxes[i] = b
    if mode == "pair":
        lam, drawn, cut, boxes = (np.concatenate((a, a[::-1])) for a in (lam, drawn, cut, boxes))
    return lam, drawn, cut, boxes


def images(rng, N, H, W):
    return [rng.integers(0, 256, (3, H, W), dtype=np.uint8) for _ in range(N)]


def area(b):
    return max(b[1] - b[0], 0) * max(b[3] - b[2], 0)


# the properties the first draw after the seed must have; (lam, drawn, cut, boxes) per sample, H and W of the case
def _elem_all_kinds(lam, drawn, cut, boxes, H, W):
    """at once: a mixup row, a row left alone (lam == 1 by `prob`), and a CutMix row whose box the border cut short -- so its lam was
    corrected -- with xl and xh both inside a 16-pixel vector"""
    mixup = any(l < 1. and not c for l, c in zip(lam, cut))
    alone = any(d == 1. for d in drawn)
    clipped = False
    for l, d, c, b in zip(lam, drawn, cut, boxes):
        if c and d != 1. and area(b):
            cut_h, cut_w = int(H * np.sqrt(1 - d)), int(W * np.sqrt(1 - d))
            short = b[1] - b[0] < 2 * (cut_h // 2) or b[3] - b[2] < 2 * (cut_w // 2)
            clipped |= bool(short and b[2] % 16 and b[3] % 16 and l != d)
    return mixup and alone and clipped


def _two_boxes(lam, drawn, cut, boxes, H, W):
    got = {tuple(b) for d, c, b in zip(drawn, cut, boxes) if c and d != 1. and area(b)}
    return len(got) >= 2


def _mixup_and_cutmix(lam, drawn, cut, boxes, H, W):
    return any(l < 1. and not c for l, c in zip(lam, cut)) and any(c and d != 1. and area(b) for d, c, b in zip(drawn, cut, boxes))


def _mixed(lam, drawn, cut, boxes, H, W):
    return lam[0] < 1.


def _empty_box(lam, drawn, cut, boxes, H, W):
    """a CutMix row whose box came out empty: its corrected lam is 1 although a lam != 1 was drawn; next to it, a row that is mixed"""
    return any(c and d != 1. and l == 1. and not area(b) for l, d, c, b in zip(lam, drawn, cut, boxes)) and any(l < 1. for l in lam)


# name, mode, N, H, W, num_classes, labels, settings, property
CASES = [
    ("elem_vec", "elem", 6, 16, 32, 37, [3, 17, 5, 9, 20, 3], dict(prob=0.5), _elem_all_kinds),  # y_0 == y_5
    ("elem_rows", "elem", 6, 8, 24, 37, [0, 36, 5, 11, 2, 8], {}, _two_boxes),  # 16-pixel vectors cross the ends of 24-pixel rows
    ("elem_odd", "elem", 4, 7, 9, 1000, [1, 2, 2, 500], {}, _mixup_and_cutmix),  # the element path
    ("pair_vec", "pair", 4, 16, 32, 37, [7, 7, 30, 8], {}, _mixup_and_cutmix),
    ("pair_odd", "pair", 2, 7, 9, 37, [0, 9], {}, _mixed),
    ("elem_empty_box", "elem", 4, 16, 32, 37, [1, 2, 3, 4], {}, _empty_box),
]


def find_seed(mx, mode, kw, N, H, W, want):
    for seed in range(10000):
        collate, rec = recording_collate(mx, mode, **kw)
        np.random.seed(seed)
        collate([(np.zeros((3, H, W), dtype=np.uint8), 0) for _ in range(N)])
        if want(*finish(rec[0], mode), H, W):
            return seed
    raise RuntimeError("no seed found")


def main(ref):
    mx = load(os.path.join(ref, "datasets", "mixup.py"), "ref_mixup")
    ce = load(os.path.join(ref, "loss", "cross_entropy.py"), "ref_cross_entropy")
    draws = {"seed": SEED, "img_shape": DRAW_SHAPE, "settings": {}}
    for mode in ("elem", "pair"):
        for name, kw in SETTINGS.items():
            collate, rec = recording_collate(mx, mode, **kw)
            np.random.seed(SEED)
            for _ in range(N_DRAWS):
                collate([(np.zeros(DRAW_SHAPE[1:], dtype=np.uint8), 0) for _ in range(DRAW_SHAPE[0])])
            batches = []
            for r in rec:
                lam, _, cut, boxes = finish(r, mode)
                batches.append(dict(lam_bits=[int(v) for v in lam.view(np.int32)], use_cutmix=[bool(v) for v in cut],
                                    boxes=[[int(v) for v in b] for b in boxes]))
            draws["settings"][f"{mode}_{name}"] = dict(kwargs=dict(RECIPE, mode=mode, **kw), draws=batches)
            print(mode, name, "CutMix samples", sum(sum(b["use_cutmix"]) for b in batches), "lam == 1 samples",
                  sum(sum(v == 0x3f800000 for v in b["lam_bits"]) for b in batches))
    with open(os.path.join(HERE, "mix_modes_draws.json"), "w") as f:
        json.dump(draws, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")

    out, meta = {}, {}
    soft = ce.SoftTargetCrossEntropy()
    for i, (name, mode, N, H, W, K, labels, kw, want) in enumerate(CASES):
        kw = dict(kw, num_classes=K)
        seed = find_seed(mx, mode, kw, N, H, W, want)
        collate, rec = recording_collate(mx, mode, **kw)
        rng = np.random.Generator(np.random.PCG64(2000 + i))
        x = np.stack(images(rng, N, H, W))
        np.random.seed(seed)
        mixed, target = collate([(img.copy(), y) for img, y in zip(x, labels)])  # (the pair collate swaps patches inside its inputs)
        lam, _, cut, boxes = finish(rec[0], mode)
        assert want(*finish(rec[0], mode), H, W)
        assert target.dtype == torch.float32 and mixed.dtype == torch.uint8 and lam.dtype == np.float32
        meta[name] = dict(mode=mode, N=N, H=H, W=W, K=K, seed=seed, kwargs=dict(RECIPE, mode=mode, **kw))
        logits = torch.from_numpy(3.0 * rng.standard_normal((N, K))).float()
        out[f"{name}__x"], out[f"{name}__labels"] = x, np.asarray(labels, dtype=np.int64)
        out[f"{name}__mixed"], out[f"{name}__target"] = mixed.numpy(), target.numpy()
        out[f"{name}__lam"], out[f"{name}__use_cutmix"], out[f"{name}__boxes"] = lam, cut, boxes
        out[f"{name}__logits"] = logits.numpy()
        for prec, lg, dt in (("f32", logits, torch.float32), ("f64", logits, torch.float64),
                             ("bf16_f64", logits.bfloat16().float(), torch.float64)):
            loss, grad, rows = loss_and_grad(soft, lg, target, dt)
            out[f"{name}__soft_loss_{prec}"], out[f"{name}__soft_grad_{prec}"], out[f"{name}__soft_rows_{prec}"] = loss, grad, rows
        print(name, meta[name], "lam", lam.tolist(), "cut", cut.tolist(), "boxes", boxes.tolist())
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    write_npz(os.path.join(HERE, "mix_modes.npz"), out)
    print("mix_modes.npz", os.path.getsize(os.path.join(HERE, "mix_modes.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
