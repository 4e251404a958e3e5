"""Fixture for the validation scoring (csrc/eval_score.hip, cotnet_amd/evaler.py), recorded from the reference's own code.

    python tests/golden/make_golden_eval.py /path/to/reference

loads the reference's `accuracy` from `utils/meters.py` where it lies, by file path -- the modules it imports at its top (`config`,
`utils.timer`, `utils.logger`, `utils.distributed`) are stubbed in sys.modules for the load; `accuracy` itself uses none of them -- runs it
on the CPU and writes DATA only, tests/golden/eval_score.npz.  Per case:

  logits, labels            seeded fp32 logits [N, K] (3 x standard normal) and int64 labels; on the rows the case names, the target logit is
                            then set halfway between two of the row's other logits, so that the target has a chosen rank
  f32_top1, f32_top5        the reference's `accuracy(logits, labels, topk=(1, 5))`
  f32_ce_sum_f64, _rows_f64 F.cross_entropy(reduction='sum') and (reduction='none') evaluated in fp64, and
  f32_ce_sum_f32, _rows_f32 the same evaluated in fp32: the tests' allowance is a multiple of the difference
  bf16_*                    all of the above on the logits rounded to bf16 (what a mixed-precision model hands over)

and `ties__*`: hand-made rows with the target tied at, across and away from the fifth place, with the reference's two counts on them.

`torch.topk` places equal values as it pleases, so a case must not depend on it: seeds are scanned upwards until, in the fp32 logits AND in
the bf16-rounded ones, no row holds a value equal to its target in another column (rounded rows of 1000 normal values do hold duplicates;
they must not involve the target) and every chosen rank came out as chosen.  The file states the property, not a magic seed.  The .npz is
written with fixed zip timestamps: a second run gives the same bytes.
"""
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name, N, K, labels, the rank the target is given per row (None: as drawn).  Ranks 0, 1, 4, 5 and 6 -- each side of the top-1 and top-5
# thresholds -- occur, one label sits in column 0 and one in column K - 1 of every case
CASES = [
    ("n4_k1000", 4, 1000, [0, 999, 417, 3], [0, 5, None, 1]),
    ("n7_k37", 7, 37, [36, 0, 5, 11, 20, 7, 7], [4, 6, 0, 1, 5, None, None]),
    ("n3_k5", 3, 5, [0, 4, 2], [4, 0, None]),
    ("n2_k1001", 2, 1001, [1000, 0], [1, 6]),
]

# hand-made rows whose target IS tied (K = 8; every value is a bf16 number): at, across and away from the fifth place.  The reference's
# counts on them are recorded only to be bracketed -- topk may place the tied target on either side
TIES = [  # label, row
    (5, [9, 8, 7, 6, 5, 5, 1, 0]),   # tied for places 4 / 5 with a LOWER column: rank 5 by the stable order, a top-5 miss
    (4, [9, 8, 7, 6, 5, 5, 1, 0]),   # the same tie, the target in the lower column: rank 4, a hit
    (6, [9, 8, 7, 5, 5, 5, 5, 0]),   # four equal values across places 3 .. 6, the target last of them: rank 6
    (3, [9, 8, 7, 5, 5, 5, 5, 0]),   # ... the target first of them: rank 3
    (1, [7, 7, 1, 1, 1, 0, 0, 0]),   # tied for the first place behind a lower column: rank 1, no top-1 hit
    (0, [7, 7, 1, 1, 1, 0, 0, 0]),   # ... in front: rank 0
    (7, [3, 3, 2, 2, 1, 1, 0, 5]),   # ties away from the target: rank 0
    (2, [4, 4, 4, 4, 4, 4, 4, 4]),   # a constant row: rank = the label
]


def load_accuracy(ref):
    """the reference's utils/meters.py, loaded by path with its top-level imports stubbed"""
    stubs = {name: types.ModuleType(name) for name in ("config", "utils", "utils.timer", "utils.logger", "utils.distributed")}
    stubs["config"].cfg = None
    stubs["utils.timer"].Timer = object
    stubs["utils.logger"].logger_info = print
    stubs["utils.distributed"].sum_tensor = None
    stubs["utils"].distributed = stubs["utils.distributed"]
    stubs["utils"].__path__ = []
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("ref_meters", os.path.join(ref, "utils", "meters.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.accuracy


def rank_by_rule(logits, labels):
    """the target's place in a stable descending sort (no NaN here): #greater + #equal in a lower column"""
    t = logits.gather(1, labels.view(-1, 1))
    cols = torch.arange(logits.shape[1]).view(1, -1)
    return ((logits > t) | ((logits == t) & (cols < labels.view(-1, 1)))).sum(1)


def ties_with_target(logits, labels):
    t = logits.gather(1, labels.view(-1, 1))
    return int((logits == t).sum()) - len(labels)


def draw(seed, N, K, labels, want):
    rng = np.random.Generator(np.random.PCG64(seed))
    logits = torch.from_numpy(3.0 * rng.standard_normal((N, K))).float()
    for n, (y, r) in enumerate(zip(labels, want)):
        if r is None:
            continue
        others = torch.cat([logits[n, :y], logits[n, y + 1:]]).sort(descending=True).values
        # exactly r other logits are greater
        logits[n, y] = others[0] + 1.0 if r == 0 else others[-1] - 1.0 if r == len(others) else (others[r - 1] + others[r]) / 2
    return logits


def find_seed(N, K, labels, want):
    lab = torch.tensor(labels, dtype=torch.int64)
    for seed in range(10000):
        logits = draw(seed, N, K, labels, want)
        ok = True
        for x in (logits, logits.bfloat16().float()):
            ranks = rank_by_rule(x, lab).tolist()
            ok = ok and ties_with_target(x, lab) == 0 and all(r is None or r == g for r, g in zip(want, ranks))
        if ok:
            return seed
    raise RuntimeError("no seed found")


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
    accuracy = load_accuracy(ref)
    ce = torch.nn.functional.cross_entropy
    out, meta = {}, {}
    for name, N, K, labels, want in CASES:
        seed = find_seed(N, K, labels, want)
        logits = draw(seed, N, K, labels, want)
        lab = torch.tensor(labels, dtype=torch.int64)
        meta[name] = dict(N=N, K=K, seed=seed, want_ranks=want)
        out[f"{name}__logits"], out[f"{name}__labels"] = logits.numpy(), lab.numpy()
        for tag, x in (("f32", logits), ("bf16", logits.bfloat16().float())):
            top1, top5 = accuracy(x, lab, topk=(1, 5))
            out[f"{name}__{tag}_top1"], out[f"{name}__{tag}_top5"] = np.int64(int(top1)), np.int64(int(top5))
            for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
                out[f"{name}__{tag}_ce_sum_{prec}"] = ce(x.to(dt), lab, reduction="sum").numpy()
                out[f"{name}__{tag}_ce_rows_{prec}"] = ce(x.to(dt), lab, reduction="none").numpy()
        print(name, meta[name], "top1 / top5", int(out[f"{name}__f32_top1"]), int(out[f"{name}__f32_top5"]), "bf16",
              int(out[f"{name}__bf16_top1"]), int(out[f"{name}__bf16_top5"]))
    tl = torch.tensor([r for _, r in TIES], dtype=torch.float32)
    ty = torch.tensor([y for y, _ in TIES], dtype=torch.int64)
    assert torch.equal(tl.bfloat16().float(), tl) and ties_with_target(tl, ty) > 0
    top1, top5 = accuracy(tl, ty, topk=(1, 5))
    out["ties__logits"], out["ties__labels"] = tl.numpy(), ty.numpy()
    out["ties__top1"], out["ties__top5"] = np.int64(int(top1)), np.int64(int(top5))
    print("ties: the reference counts", int(top1), int(top5), "ranks by the rule", rank_by_rule(tl, ty).tolist())
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "eval_score.npz")
    write_npz(path, out)
    print("eval_score.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
