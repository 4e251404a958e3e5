"""Fixtures for the recipe's mixup / CutMix and soft-target loss, recorded from the reference's own code.

    python tests/golden/make_golden_recipe.py /path/to/reference

loads the reference's `datasets/mixup.py` and `loss/cross_entropy.py` where they lie, by file path (importing the `datasets` package would
pull in torchvision), runs `FastCollateMixup(mode='batch')`, `SoftTargetCrossEntropy` and `LabelSmoothingCrossEntropy` on the CPU and writes
DATA only:

  recipe_draws.json   (a) for np.random.seed(SEED): (lam, use_cutmix, box, lam as drawn) of 64 consecutive batches of 2 x 3 x 224 x 224 images under three
                      settings -- the recipes' (mixup 0.8, cutmix 1.0, prob 1, switch 0.5), the same with prob 0.5, and cutmix_minmax [0.2, 0.8]
  recipe_mix.npz      (b) per case: the uint8 inputs, the integer labels, the reference's mixed uint8 output and its dense target, with the
                      parameters it drew; (c) seeded fp32 logits, the reference's loss (mean and per row) and autograd gradient on them in
                      fp32 and in fp64, the same on the bf16-rounded logits in fp64, and LabelSmoothingCrossEntropy(0.1) on the hard labels
                      in fp32 and fp64.

The cases' seeds are FOUND here, by scanning seeds upwards until the reference's own draw has the property the case is about (a box
clipped by the border, lam == 1, ...), so the file states the property, not a magic number.  The .npz is written with fixed zip
timestamps: a second run gives the same bytes.
"""
import importlib.util
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240
RECIPE = dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', label_smoothing=0.1)
SETTINGS = {"recipe": {}, "prob_half": dict(prob=0.5), "minmax": dict(cutmix_minmax=[0.2, 0.8])}
N_DRAWS = 64


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recording_collate(mx, **kw):
    """FastCollateMixup whose draw is written down: `rec` receives (lam, use_cutmix, box) of every batch it collates"""
    rec = []
    real_bbox = mx.__dict__.setdefault("_unrecorded_bbox", mx.cutmix_bbox_and_lam)

    class Recording(mx.FastCollateMixup):
        def _params_per_batch(self):
            lam, use_cutmix = super()._params_per_batch()
            rec.append([float(lam), bool(use_cutmix), [0, 0, 0, 0], float(lam)])  # (the last: lam as drawn, before the correction)
            return lam, use_cutmix

    def bbox(*a, **k):
        box, lam = real_bbox(*a, **k)
        rec[-1][0], rec[-1][2] = float(lam), [int(v) for v in box]
        return box, lam
    mx.cutmix_bbox_and_lam = bbox
    kw = dict(RECIPE, **kw)
    if kw["cutmix_minmax"] is None:
        kw["cutmix_minmax"] = ()  # (the reference's constructor takes len() of it)
    return Recording(**kw), rec


def images(rng, N, H, W):
    return [(rng.integers(0, 256, (3, H, W), dtype=np.uint8), 0) for _ in range(N)]


# (b) / (c): name, N, H, W, num_classes, labels, settings, the property the first draw after the seed must have
def _clipped_unaligned(lam, cut, box, drawn):
    """a CutMix box that the image border (16 x 32) cut short -- so lam was corrected -- whose xl and xh both fall inside a 16-pixel vector"""
    yl, yh, xl, xh = box
    cut_h = int(16 * np.sqrt(1 - drawn))
    return cut and 0 < yh - yl < 2 * (cut_h // 2) and xl % 16 and xh % 16 and xh > xl and lam != drawn


CASES = [
    ("mixup_vec", 4, 16, 32, 1000, [3, 17, 999, 3], {}, lambda lam, cut, box, drawn: not cut and lam < 1.),  # y_0 == y_3
    ("cutmix_vec", 4, 16, 32, 37, [0, 36, 5, 11], {}, _clipped_unaligned),
    ("cutmix_elem", 4, 7, 9, 1000, [1, 2, 2, 500], {}, lambda lam, cut, box, drawn: cut and box[1] > box[0] and box[3] > box[2]),
    ("mixup_elem", 4, 7, 9, 37, [7, 7, 7, 8], {}, lambda lam, cut, box, drawn: not cut and lam < 1.),
    ("lam1_n2", 2, 16, 32, 10, [4, 9], dict(prob=0.5), lambda lam, cut, box, drawn: lam == 1.),
    ("mixup_n2", 2, 7, 9, 10, [0, 9], {}, lambda lam, cut, box, drawn: not cut and lam < 1.),
    ("minmax_vec", 4, 16, 32, 37, [1, 2, 3, 4], dict(cutmix_minmax=[0.2, 0.8]), lambda lam, cut, box, drawn: cut),
]


def find_seed(mx, kw, shape, want):
    for seed in range(10000):
        collate, rec = recording_collate(mx, **kw)
        np.random.seed(seed)
        collate([(np.zeros(shape, dtype=np.uint8), 0)] * 2)
        if want(*rec[0]):
            return seed
    raise RuntimeError("no seed found")


def loss_and_grad(fn, logits, target, dtype):
    """-> the reference's mean loss, its autograd gradient, and the loss of every row (the module applied to one row at a time: the
    mean of one row is that row's loss)"""
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    t = target if target.dtype == torch.int64 else target.to(dtype)
    loss = fn(x, t)
    loss.backward()
    with torch.no_grad():
        rows = torch.stack([fn(x[i:i + 1], t[i:i + 1]) for i in range(len(x))])
    return loss.detach().numpy(), x.grad.numpy(), rows.numpy()


def write_npz(path, arrays):
    """np.savez_compressed with the zip members' timestamps fixed, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main(ref):
    mx = load(os.path.join(ref, "datasets", "mixup.py"), "ref_mixup")
    ce = load(os.path.join(ref, "loss", "cross_entropy.py"), "ref_cross_entropy")
    draws = {"seed": SEED, "img_shape": [2, 3, 224, 224], "settings": {}}
    for name, kw in SETTINGS.items():
        collate, rec = recording_collate(mx, **kw)
        batch = [(np.zeros((3, 224, 224), dtype=np.uint8), 0)] * 2
        np.random.seed(SEED)
        for _ in range(N_DRAWS):
            collate(batch)
        draws["settings"][name] = dict(kwargs=dict(RECIPE, **kw), draws=rec)
        print(name, "cutmix batches", sum(r[1] for r in rec), "lam == 1 batches", sum(r[0] == 1. for r in rec))
    with open(os.path.join(HERE, "recipe_draws.json"), "w") as f:
        json.dump(draws, f, indent=0, sort_keys=True)
        f.write("\n")

    out, meta = {}, {}
    soft, smooth = ce.SoftTargetCrossEntropy(), ce.LabelSmoothingCrossEntropy(0.1)
    for i, (name, N, H, W, K, labels, kw, want) in enumerate(CASES):
        seed = find_seed(mx, dict(kw, num_classes=K), (3, H, W), want)
        collate, rec = recording_collate(mx, num_classes=K, **kw)
        rng = np.random.Generator(np.random.PCG64(1000 + i))
        batch = [(img, y) for (img, _), y in zip(images(rng, N, H, W), labels)]
        np.random.seed(seed)
        mixed, target = collate(batch)
        lam, cut, box, _ = rec[0]
        meta[name] = dict(N=N, H=H, W=W, K=K, seed=seed, lam=lam, use_cutmix=cut, box=box, kwargs=dict(RECIPE, num_classes=K, **kw))
        logits = torch.from_numpy(3.0 * rng.standard_normal((N, K))).float()
        lab = torch.tensor(labels, dtype=torch.int64)
        out[f"{name}__x"] = np.stack([b[0] for b in batch])
        out[f"{name}__labels"] = lab.numpy()
        out[f"{name}__mixed"] = mixed.numpy()
        out[f"{name}__target"] = target.numpy()
        out[f"{name}__logits"] = logits.numpy()
        assert target.dtype == torch.float32 and mixed.dtype == torch.uint8
        for tag, fn, tg in (("soft", soft, target), ("ls", smooth, lab)):
            for prec, x, dt in (("f32", logits, torch.float32), ("f64", logits, torch.float64),
                                ("bf16_f64", logits.bfloat16().float(), torch.float64)):
                loss, grad, rows = loss_and_grad(fn, x, tg, dt)
                out[f"{name}__{tag}_loss_{prec}"], out[f"{name}__{tag}_grad_{prec}"] = loss, grad
                out[f"{name}__{tag}_rows_{prec}"] = rows
        print(name, meta[name])
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    write_npz(os.path.join(HERE, "recipe_mix.npz"), out)
    print("recipe_mix.npz", os.path.getsize(os.path.join(HERE, "recipe_mix.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
