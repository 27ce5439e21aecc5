"""CPU-side tests (-m "not gpu"): oracle vs committed golden fixtures, the drop-in boundary's
state_dict contract, C-ABI symbol coverage, host logic.  No GPU compute is called."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import cilrs_oracle as O


def test_oracle_known_answers(golden_dir):
    m = O.CILRSOracle()
    assert sum(p.numel() for p in m.parameters()) == 22_421_453      # notebook.ipynb:52
    keys = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    sd = m.state_dict()
    assert keys["n_entries"] == 250 == len(sd)
    for e, (k, v) in zip(keys["entries"], sd.items()):
        assert e["name"] == k and tuple(e["shape"]) == tuple(v.shape)
        assert e["dtype"] == str(v.dtype).replace("torch.", "")
    # checkpoint size 256.9 MB = params + exp_avg + exp_avg_sq in fp32 (notebook.ipynb:306)
    assert abs(3 * 22_421_453 * 4 / 2 ** 20 - 256.9) < 0.6


def test_portable_weights_reproducible(golden_dir):
    m = O.CILRSOracle()
    sd = O.portable_state_dict(m.state_dict(), 0)
    chk = json.load(open(os.path.join(golden_dir, "portable_weights_check.json")))
    assert float(sd["visual_encoder.0.weight"].double().sum()) == chk["first"]
    assert float(sd["speed_predictor.5.bias"].double().sum()) == chk["last"]


def test_oracle_forward_eval_matches_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "forward_eval_b4.npz"))
    m = O.build_oracle(0).eval()
    img, spd, _, _, _ = O.synthetic_batch(4, seed=int(g["seed"]))
    assert float(img.double().sum()) == float(g["image_sum"])
    with torch.no_grad():
        c, s = m(img, spd, torch.from_numpy(g["command"]))
    # same torch build -> bit-identical; allow last-ulp slack for other CPU kernels
    assert np.abs(c.numpy() - g["controls"]).max() <= 2e-6
    assert np.abs(s.numpy() - g["pred_speed"]).max() <= 2e-6


def test_oracle_train_step_matches_golden(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "step_cfgB_b8.json")))
    m = O.build_oracle(0)
    opt = O.make_optimizer(m, O.CONFIG_B)
    imgs, spds, cmds, tgts = O.synthetic_batch(8, seed=ref["seeds"][0])[:4]
    ld, gn = O.train_step(m, opt, O.CONFIG_B, imgs, spds, cmds, tgts)
    for k, v in ref["steps"][0]["loss"].items():
        assert abs(ld[k] - v) <= 1e-5 * max(1.0, abs(v))
    assert abs(gn - ref["steps"][0]["gnorm"]) <= 1e-4 * ref["steps"][0]["gnorm"]
    for n, p in m.named_parameters():
        want = ref["steps"][0]["params"][n]
        assert abs(float(p.detach().double().norm()) - want["l2"]) <= 1e-5 * max(1.0, want["l2"])


def test_infer_pipeline_matches_golden(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "infer_pipeline.json")))
    frame = np.floor(O._hash_u01(g["frame_seed"], g["frame_stream"], 88 * 200 * 3) * 256)
    frame = frame.astype(np.uint8).reshape(88, 200, 3)
    assert int(frame.astype(np.int64).sum()) == g["frame_sum"]
    m = O.build_oracle(0)
    case = g["cases"][0]
    out = O.predict_controls(m, frame, case["speed_kmh"], case["command"])
    assert np.abs(np.array(out) - np.array(case["out"])).max() <= 2e-5


# ---- drop-in boundary -------------------------------------------------------------------------
def test_module_state_dict_contract(golden_dir):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=0.0)
    keys = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    sd = m.state_dict()
    assert [e["name"] for e in keys["entries"]] == list(sd.keys())
    for e in keys["entries"]:
        assert tuple(e["shape"]) == tuple(sd[e["name"]].shape)
        assert e["dtype"] == str(sd[e["name"]].dtype).replace("torch.", "")
    assert sum(p.numel() for p in m.parameters()) == 22_421_453
    # both directions of the checkpoint contract (autonomous_drive.py:497, strict)
    o = O.CILRSOracle()
    o.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(O.portable_state_dict(o.state_dict(), 3), strict=True)
    assert torch.equal(m.state_dict()["control_branches.2.3.weight"],
                       O.portable_state_dict(o.state_dict(), 3)["control_branches.2.3.weight"])


def test_forward_fails_loudly_without_gpu():
    from cilrs_mi355 import CILRS
    m = CILRS()
    x = torch.zeros(1, 3, 88, 200)
    with pytest.raises(RuntimeError, match="no CPU fallback|ROCm device"):
        m(x, torch.zeros(1), torch.zeros(1, dtype=torch.long))


def test_capi_exports_every_declared_symbol():
    from cilrs_mi355 import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cilrs_hip.h")).read()
    declared = set(re.findall(r"\b(cilrs_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in cilrs_hip.h but not exported"
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)


def test_arena_layout_matches_module():
    from cilrs_mi355 import CILRS
    from cilrs_mi355.engine import _layout, segment_ranges
    from cilrs_mi355 import _lib as L
    params, bns = _layout()
    m = CILRS()
    assert [p[0] for p in params] == [n for n, _ in m.named_parameters()]
    assert [tuple(p[3]) for p in params] == [tuple(p.shape) for p in m.parameters()]
    assert sum(p[2] for p in params) == 22_421_453 == L.lib().cilrs_param_count()
    assert len(bns) == 36
    mods = dict(m.named_modules())
    for prefix, ch, _, _ in bns:
        assert mods[prefix].num_features == ch
    # offsets: 16-byte aligned, non-overlapping, in order
    end = 0
    for _, off, numel, _ in params:
        assert off % 4 == 0 and off >= end
        end = off + numel
    assert end <= L.lib().cilrs_param_arena_floats()
    segs = segment_ranges()
    covered = sorted(segs)
    assert covered[0][0] == 0 and covered[-1][1] == L.lib().cilrs_param_arena_floats()
    for (b0, e0), (b1, e1) in zip(covered, covered[1:]):
        assert e0 == b1


def test_bucket_plan_covers_arena():
    from cilrs_mi355.engine import segment_ranges
    from cilrs_mi355.parallel import bucket_plan
    from cilrs_mi355 import _lib as L
    b = bucket_plan(segment_ranges())
    spans = sorted((x[1], x[2]) for x in b)
    assert spans[0][0] == 0 and spans[-1][1] == L.lib().cilrs_param_arena_floats()
    for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
        assert e0 == b1
    assert [x[0] for x in b] == [1, 2, 5]          # issued in backward order


# ---- data parallel host logic on CPU (gloo, world_size 2) ---------------------------------------
def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cilrs_mi355.engine import segment_ranges
    from cilrs_mi355.parallel import BucketedAllReduce, bucket_plan
    from cilrs_mi355 import _lib as L
    n = L.lib().cilrs_param_arena_floats()
    g = torch.Generator().manual_seed(100 + rank)
    flat = torch.randn(n, generator=g)
    mine = flat.clone()
    segs = segment_ranges()
    red = BucketedAllReduce(flat, buckets=bucket_plan(segs))

    class FakeEngine:                       # stands in for the HIP backward: grads already there
        calls = []

        def run_backward(self, plan, dc, dp, a, b):
            self.calls.append((a, b))

    eng = FakeEngine()
    red.backward_and_reduce(eng, None, None, None)
    assert eng.calls == [(0, 2), (2, 3), (3, 6)]
    others = [torch.randn(n, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)]
    want = sum(others)
    ok = bool(torch.allclose(flat, want, atol=1e-5)) and not torch.equal(flat, mine)
    # the per-bucket hook (the Trainer updates a bucket's parameter range there): called once per
    # bucket, in issue order, with the bucket's range, and the bucket is REDUCED when it is called
    flat.copy_(mine)
    seen = []

    def after(i, b, e):
        seen.append((i, b, e, bool(torch.allclose(flat[b:e], want[b:e], atol=1e-5))))
    red.backward_and_reduce(eng, None, None, None, after_bucket=after)
    plan = bucket_plan(segs)
    ok = ok and [(i, b, e) for i, b, e, _ in seen] == [(i, b, e) for i, (_, b, e) in enumerate(plan)] \
        and all(x[3] for x in seen) and not red._pending
    q.put((rank, ok, red.world_size))
    dist.destroy_process_group()


def test_bucketed_allreduce_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(r[0] for r in res) == [0, 1]
    assert all(r[1] for r in res) and all(r[2] == 2 for r in res)


def test_dp_equivalence_semantics_with_oracle():
    """an N-GPU step == per-shard gradients (per-replica BN statistics) averaged,
    then ONE Adam step -- not a single 2x-batch step.  Pins the semantics the GPU path follows."""
    torch.manual_seed(0)
    m = O.build_oracle(0)
    shards = [O.synthetic_batch(2, seed=60 + r)[:4] for r in range(2)]
    grads = []
    for imgs, spds, cmds, tgts in shards:
        m.zero_grad()
        m.train()
        pc, ps = m(imgs, spds, cmds)
        loss, _ = O.compute_loss(O.CONFIG_A, pc, tgts, ps, spds)
        loss.backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    avg = [(a + b) / 2 for a, b in zip(*grads)]
    big = [torch.cat([a, b]) for a, b in zip(*shards)]
    m.zero_grad()
    pc, ps = m(*big[:3])
    loss, _ = O.compute_loss(O.CONFIG_A, pc, big[3], ps, big[1])
    loss.backward()
    diff = max(float((p.grad - a).abs().max()) for p, a in zip(m.parameters(), avg))
    assert diff > 1e-4          # batch statistics differ: DP is NOT one big batch


def test_evaluation_report_oracle_schema_and_identities(golden_dir):
    """The reference ships evaluation_report.json but not its generator: pin the oracle's report
    on the published key structure and on the identities the published numbers satisfy."""
    import eval_report as ER
    g = json.load(open(os.path.join(golden_dir, "evaluation_report_schema.json")))
    for name, (mse, rmse) in g["mse_rmse"].items():          # published: RMSE == sqrt(MSE)
        assert abs(rmse - mse ** 0.5) <= 1e-12, name
    assert sum(g["per_command_n"].values()) == g["val_samples"]
    rng = np.random.default_rng(5)
    n = 500
    tc = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    ts = rng.uniform(0, 1, n).astype(np.float32)
    pc = (tc + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    ps = (ts + rng.normal(0, 0.02, n)).astype(np.float32)
    cmd = rng.integers(0, 4, n)
    rep = ER.evaluation_report(pc, ps, tc, ts, cmd, checkpoint_epoch=3)

    def keys(d):
        return {k: (keys(v) if isinstance(v, dict) else type(v).__name__) for k, v in d.items()}
    assert keys(rep) == g["schema"]
    # known answers: numpy's own estimators
    assert abs(rep["overall_metrics"]["Steer"]["Correlation"]
               - np.corrcoef(pc[:, 0].astype(np.float64), tc[:, 0].astype(np.float64))[0, 1]) < 1e-12
    assert abs(rep["overall_metrics"]["Speed"]["RMSE"] ** 2 - rep["overall_metrics"]["Speed"]["MSE"]) < 1e-15
    assert sum(v["n"] for v in rep["per_command_metrics"].values()) == rep["val_samples"] == n
    b = rep["steer_accuracy_buckets"]
    assert b["within_0.01"] <= b["within_0.02"] <= b["within_0.05"] <= b["within_0.1"] <= 1.0
    p = rep["steer_percentiles"]
    assert p["P50"] <= p["P75"] <= p["P90"] <= p["P95"] <= p["P99"]
    # weighted per-command steer MAE reassembles the overall one
    tot = sum(v["n"] * v["steer_mae"] for v in rep["per_command_metrics"].values()) / n
    assert abs(tot - rep["overall_metrics"]["Steer"]["MAE"]) < 1e-14


def test_oracle_resize_restatement(golden_dir):
    """OpenCV 8-bit INTER_LINEAR restated (cv2 absent -> parity unpinned): golden digest, and the
    properties the algorithm guarantees -- identity at equal size, constants preserved, within one
    grey level of exact bilinear sampling, channel order untouched."""
    import hashlib
    g = json.load(open(os.path.join(golden_dir, "camera_pipeline.json")))
    cam = np.floor(O._hash_u01(g["frame_seed"], g["frame_stream"], 600 * 800 * 4) * 256)
    cam = cam.astype(np.uint8).reshape(600, 800, 4)
    rgb = np.ascontiguousarray(cam[:, :, :3])
    small = O.resize_bilinear_u8(rgb)
    assert small.shape == (88, 200, 3) and small.dtype == np.uint8
    assert hashlib.sha256(small.tobytes()).hexdigest() == g["resized_sha256"]
    assert small[0, :8].reshape(-1).tolist() == g["resized_row0"]
    same = O.resize_bilinear_u8(small)
    assert same is not small and np.array_equal(same, small)
    assert np.unique(O.resize_bilinear_u8(np.full((600, 800, 3), 201, np.uint8))).tolist() == [201]
    fx = (np.arange(200) + 0.5) * 4 - 0.5
    fy = (np.arange(88) + 0.5) * (600 / 88) - 0.5
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    wx, wy = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    F = rgb.astype(np.float64)
    top = F[y0][:, x0] * (1 - wx) + F[y0][:, x0 + 1] * wx
    bot = F[y0 + 1][:, x0] * (1 - wx) + F[y0 + 1][:, x0 + 1] * wx
    assert np.abs(small - (top * (1 - wy) + bot * wy)).max() <= 1.0
    for c in range(3):
        assert np.array_equal(O.resize_bilinear_u8(rgb[:, :, c:c + 1])[:, :, 0], small[:, :, c])
    # upscaling exercises the clamped edge taps
    up = O.resize_bilinear_u8(small[:10, :12], width=31, height=23)
    assert up.shape == (23, 31, 3) and up.min() >= small[:10, :12].min()


# ---- input pipeline: host side ------------------------------------------------
CSV_COLUMNS = ["frame", "image_filename", "steer", "throttle", "brake", "speed_kmh",
               "speed_normalized", "high_level_command", "command_name", "position_x",
               "position_y", "position_z", "yaw", "timestamp"]          # collect_data.py:549-564


def make_sessions(root, n_per_session=(7, 5), seed=3):
    """A dataset in the reference's on-disk format (collect_data.py:545-564, 683-716)."""
    import csv
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = ["LANEFOLLOW", "LEFT", "RIGHT", "STRAIGHT"]
    frames = []
    for si, n in enumerate(n_per_session):
        sdir = os.path.join(root, f"session{si + 1}")
        os.makedirs(os.path.join(sdir, "images"))
        with open(os.path.join(sdir, "measurements.csv"), "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(CSV_COLUMNS)
            for k in range(n):
                # smooth images so JPEG round trips stay close
                base = rng.integers(0, 256, (11, 25, 3), dtype=np.uint8)
                img = np.asarray(Image.fromarray(base).resize((200, 88), Image.BILINEAR))
                fn = f"frame_{k:08d}.jpg"
                Image.fromarray(img).save(os.path.join(sdir, "images", fn), quality=95)
                c = int(rng.integers(0, 4)) if k >= 4 else k
                kmh = float(rng.uniform(0, 90))
                wr.writerow([k, fn, round(float(rng.uniform(-1, 1)), 6),
                             round(float(rng.uniform(0, 1)), 6), round(float(rng.uniform(0, 1)), 6),
                             round(kmh, 2), round(kmh / 90.0, 6), c, names[c], 1.0, 2.0, 0.5, 90.0,
                             round(0.05 * k, 3)])
                frames.append(img)
    return frames


def test_sessions_reader_sampler_and_split(tmp_path):
    from cilrs_mi355 import data as D
    make_sessions(str(tmp_path), (12, 9))
    s = D.Sessions(str(tmp_path))
    assert len(s) == 21 and s.targets.shape == (21, 3) and s.command.dtype == np.int64
    assert s.paths[0].endswith(os.path.join("session1", "images", "frame_00000000.jpg"))
    assert set(s.command[:4].tolist()) == {0, 1, 2, 3}
    img = D.decode_jpeg(s.paths[0])
    assert img.shape == (88, 200, 3) and img.dtype == np.uint8
    # class weights: len / (4 * count)  (notebook.ipynb:384)
    w = D.class_balanced_weights(s.command)
    cnt = np.bincount(s.command, minlength=4)
    assert np.allclose(w, 21 / (4 * cnt[s.command]))
    # identical draws to the reference's WeightedRandomSampler (notebook.ipynb:422-423)
    from torch.utils.data import WeightedRandomSampler
    ref = list(WeightedRandomSampler(torch.DoubleTensor(w), num_samples=21, replacement=True,
                                     generator=torch.Generator().manual_seed(9)))
    got = D.weighted_indices(w, 21, torch.Generator().manual_seed(9)).tolist()
    assert got == ref
    tr, va = s.split()
    assert len(va) == 4 and len(tr) == 17 and not set(tr) & set(va)
    assert D.AUG_DTYPE.itemsize == 112          # cilrs_aug_params, include/cilrs_hip.h
    with pytest.raises(RuntimeError):
        D.augment_u8(torch.zeros(1, 88, 200, 3, dtype=torch.uint8), D.identity_params(1))


def test_augment_oracle_properties():
    import augment_oracle as AO
    from cilrs_mi355 import data as D
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)

    def rec(**kw):
        p = {k: D.identity_params(1)[0][k] for k in D.AUG_DTYPE.names}
        p = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in p.items()}
        p.update(kw)
        return p
    assert np.array_equal(AO.augment_one(f, rec()), f)
    out = AO.augment_one(f, rec(rbc_on=1, alpha=1.1, beta255=-12.75))
    want = np.clip(f.astype(np.float32) * np.float32(1.1) + np.float32(-12.75), 0, 255).astype(np.uint8)
    assert np.array_equal(out, want)
    # HSV with zero shifts only re-quantises through 8-bit HSV (half-degree hue): a few grey levels
    out = AO.augment_one(f, rec(hsv_on=1))
    assert np.abs(out.astype(int) - f.astype(int)).max() <= 5
    grey = np.full((4, 4, 3), 77, np.uint8)
    assert np.array_equal(AO.augment_one(grey, rec(hsv_on=1, hue=7.0)), grey)   # hue of grey: no-op
    # blur keeps constants, dropout zeroes its rectangle only
    assert np.array_equal(AO.augment_one(grey, rec(blur_k=5, blur_w=D.gaussian_taps(5, 1.3).tolist())), grey)
    out = AO.augment_one(f, rec(nholes=1, hole_y0=[2, 0, 0], hole_x0=[3, 0, 0], hole_y1=[6, 0, 0],
                                hole_x1=[9, 0, 0]))
    assert (out[2:6, 3:9] == 0).all() and np.array_equal(out[6:], f[6:])
    n = AO.gaussian_noise(1234, 200000)
    assert abs(float(n.mean())) < 0.01 and abs(float(n.std()) - 1.0) < 0.01
    t = D.gaussian_taps(5, 2.0)
    assert abs(t[0] + 2 * t[1] + 2 * t[2] - 1.0) < 1e-6
    # the drawn parameter distribution follows the Compose probabilities (notebook.ipynb:387-394)
    p = D.draw_aug_params(np.random.default_rng(0), 4000)
    for field, prob in (("rbc_on", 0.5), ("hsv_on", 0.3)):
        assert abs(p[field].mean() - prob) < 0.03
    assert abs((p["blur_k"] > 1).mean() - 0.2) < 0.03 and abs((p["nholes"] > 0).mean() - 0.2) < 0.03
    assert abs((p["noise_std255"] > 0).mean() - 0.3) < 0.03
    assert p["alpha"].min() >= 0.8 and p["alpha"].max() <= 1.2 and np.abs(p["hue"]).max() <= 10
    D.check_params(p, 88, 200)


# ---- round 2: launcher, rank sharding, reference-written checkpoints ---------------------------
def test_bench_self_launches_two_ranks_gloo_rehearsal():
    """`python bench.py --gpus 2` with no launcher in front starts two fresh ranks itself, relays
    rank 0's single JSON line on stdout and exits 0 (CPU rehearsal over gloo: the launcher, the
    rendezvous, the bucketed all-reduce of the real arena layout and the JSON relay -- the HIP
    engine is not involved and nothing is measured)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps",
                        "2", "--warmup", "0", "--rehearse"], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["rehearsal"] is True and out["n_gpus"] == 2 and out["n_ranks_seen"] == 2
    assert out["allreduce_sum_ok"] is True and out["value"] is None


def test_bench_launcher_propagates_rank_failure():
    """A failing rank makes `bench.py --gpus N` exit non-zero and print no result line (here: the
    product path refuses to run without a GPU; on a GPU box an RCCL error ends a rank the same
    way)."""
    import subprocess
    import sys
    if torch.cuda.is_available():
        pytest.skip("needs a box without GPUs to make the ranks fail")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps",
                        "1", "--warmup", "0"], capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.strip().startswith("{")]


_DUMP = r"""
import sys, types
import torch
sys.path.insert(0, sys.argv[1])
import bench
from cilrs_mi355 import _lib
lib = _lib.lib()
n = lib.cilrs_param_arena_floats()
g = torch.Generator().manual_seed(7)
eng = types.SimpleNamespace(n_arena=n, params=torch.randn(n, generator=g),
                            grads=torch.randn(n, generator=g),
                            bn=torch.randn(lib.cilrs_bn_arena_floats(), generator=g))
tr = types.SimpleNamespace(eng=eng, exp_avg=eng.params * 0.5, exp_avg_sq=eng.grads ** 2,
                           loss_buf=torch.arange(8, dtype=torch.float32))
bench.dump_outputs(sys.argv[2], tr)
"""


def test_bench_dump_outputs_are_float32_bounded_and_sampled_at_fixed_positions(tmp_path):
    """`bench.py --dump-outputs DIR` (here on a stand-in trainer with the real arena sizes, in a
    fresh process each time): float32 .npy files, at most 64 MB in all, and the same state gives
    the same files in two processes -- the arena sample positions do not vary from run to run."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    for d in dirs:
        r = subprocess.run([sys.executable, "-c", _DUMP, root, d], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) == sorted(
        f"{k}.npy" for k in ("loss", "bn_running", "params", "exp_avg", "exp_avg_sq", "grads"))
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in names) <= 64 * 2 ** 20
    for f in names:
        a, b = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    assert np.array_equal(np.load(os.path.join(dirs[0], "loss.npy")), np.arange(6))


def test_batch_loader_rank_shards_are_disjoint_and_cover_the_single_process_draw():
    """SURVEY.md 8e rank-strided sampling: with one shared sampler stream (equal seeds) the two
    ranks' epoch orders are disjoint POSITIONS of the single-process WeightedRandomSampler draw
    (notebook.ipynb:421-431) and together are exactly that draw; both run the same step count."""
    from cilrs_mi355.data import BatchLoader

    class FakeSessions:
        command = np.array(([0] * 50 + [1] * 27 + [2] * 14 + [3] * 9) * 11, dtype=np.int64)

    idx = np.arange(len(FakeSessions.command))[::-1].copy()
    bs = 16
    single = BatchLoader(FakeSessions, idx, 2 * bs, "cpu", train=True, seed=7)
    want = single._order()
    parts = [BatchLoader(FakeSessions, idx, bs, "cpu", train=True, seed=7, rank=r, world_size=2)
             for r in range(2)]
    orders = [p._order() for p in parts]
    assert len(parts[0]) == len(parts[1]) == len(single) and len(single) > 0
    assert len(orders[0]) == len(orders[1]) == len(want) // 2
    inter = np.empty(len(want), dtype=want.dtype)
    inter[0::2], inter[1::2] = orders[0], orders[1]
    assert np.array_equal(inter, want)                 # union == the single-process draw, in order
    # global batch g of the single process == rank 0's batch g + rank 1's batch g (as multisets)
    for g in range(len(single)):
        a = np.sort(want[g * 2 * bs:(g + 1) * 2 * bs])
        b = np.sort(np.concatenate([o[g * bs:(g + 1) * bs] for o in orders]))
        assert np.array_equal(a, b)
    # validation: sequential, strided, every sample exactly once, ragged tail kept
    vparts = [BatchLoader(FakeSessions, idx[:101], bs, "cpu", train=False, rank=r, world_size=2)
              for r in range(2)]
    vo = [p._order() for p in vparts]
    assert sorted(np.concatenate(vo).tolist()) == sorted(idx[:101].tolist())
    assert not set(vo[0].tolist()) & set(vo[1].tolist())
    assert [len(p) for p in vparts] == [4, 4]          # 51 and 50 samples in batches of 16
    # augmentation streams differ between ranks, sampler streams do not
    assert parts[0].rng.integers(1 << 30) != parts[1].rng.integers(1 << 30)
    with pytest.raises(ValueError):
        BatchLoader(FakeSessions, idx, bs, "cpu", train=True, rank=2, world_size=2)


def test_dropout_seed_depends_on_rank_and_step():
    from cilrs_mi355.train import dropout_seed
    seeds = {dropout_seed(1234, c, r) for c in range(1, 4) for r in range(8)}
    assert len(seeds) == 24 and all(0 <= s < 2 ** 64 for s in seeds)
    assert dropout_seed(1234, 1, 0) == (1234 * 1000003 + 1)     # rank 0 keeps round 1's stream


def test_checkpoint_written_the_reference_way_loads(tmp_path):
    """The reference saves np.float64 values (np.mean) in cmd_steer_errors / val_loss
    (notebook/notebook.ipynb:584, 631-636), which torch's weights-only unpickler rejects by
    default and for which the reference's own loader carries a numpy shim
    (autonomous_drive.py:35-44).  checkpoint.load reads such a file -- still without executing
    anything from it -- and restores the weights with strict=True (autonomous_drive.py:496-497)."""
    from cilrs_mi355 import CILRS, checkpoint
    src = O.build_oracle(3)
    opt = O.make_optimizer(src, O.CONFIG_B)
    path = str(tmp_path / "checkpoint_best.pth")
    cmd_steer_errors = {"FOLLOW": np.mean([0.01, 0.02]), "LEFT": np.mean([0.03]),
                        "RIGHT": np.mean([0.04]), "STRAIGHT": np.mean([0.05])}
    assert type(cmd_steer_errors["FOLLOW"]) is np.float64
    torch.save({"epoch": 20, "model_state_dict": src.state_dict(),
                "optimizer_state_dict": opt.state_dict(), "val_loss": np.float64(0.0538),
                "val_steer": np.float64(0.0048), "config": {"lr": 1e-4, "batch_size": 120},
                "cmd_steer_errors": cmd_steer_errors}, path)
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu", weights_only=True)     # the default loader refuses
    m = CILRS(4, 0.0)
    ck = checkpoint.load(path, m)
    assert ck["epoch"] == 20 and abs(float(ck["val_loss"]) - 0.0538) < 1e-12
    assert abs(float(ck["cmd_steer_errors"]["FOLLOW"]) - 0.015) < 1e-12
    for (k, a), (_, b) in zip(m.state_dict().items(), src.state_dict().items()):
        assert torch.equal(a, b), k
    # the allow-list covers numpy scalars only: any other global in the file is still refused
    evil = str(tmp_path / "other.pth")
    import fractions
    torch.save({"model_state_dict": src.state_dict(), "x": fractions.Fraction(1, 3)}, evil)
    with pytest.raises(Exception):
        checkpoint.load_file(evil)


def test_resnet50_variant_layout_matches_its_oracle():
    """BASELINE.json configs[3] (ResNet-50 variant; the reference has no such model): the module,
    the engine's arena layout (C-ABI variant 1) and the CPU definition agree on every parameter
    name / shape / order; the trunk has torchvision ResNet-50's parameter count without its fc."""
    import resnet50_oracle as R
    from cilrs_mi355 import CILRSResNet50
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.engine import _layout
    orc = R.CILRSResNet50Oracle()
    assert sum(p.numel() for p in orc.visual_encoder.parameters()) == R.TRUNK_PARAMS == 23_508_032
    m = CILRSResNet50(4, 0.0)
    assert list(m.state_dict().keys()) == list(orc.state_dict().keys())
    for (k, a), (_, b) in zip(m.state_dict().items(), orc.state_dict().items()):
        assert a.shape == b.shape and a.dtype == b.dtype, k
    lay, bns = _layout(1)
    assert [(n, s) for n, _, _, s in lay] == [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    lib = L.lib()
    assert lib.cilrs_num_variants() == 2
    assert lib.cilrs_variant_param_count(1) == sum(p.numel() for p in orc.parameters())
    assert lib.cilrs_variant_feature_width(1) == 2048 and lib.cilrs_variant_feature_width(0) == 512
    assert lib.cilrs_variant_num_bn(1) == len(bns) == 53
    # variant 0 through the variant API == the plain API (the reference's network)
    assert lib.cilrs_variant_param_count(0) == lib.cilrs_param_count() == 22_421_453
    assert _layout(0)[0][:3] == _layout()[0][:3]
    with pytest.raises(RuntimeError):
        m.train()(torch.zeros(1, 3, 176, 400), torch.zeros(1), torch.zeros(1, dtype=torch.long))


def test_torchvision_trunk_keys_map_onto_the_reference_wrapping():
    """ImageNet-pretrained start of the executed notebook (nb:444): a torchvision-keyed ResNet-34
    state_dict (the oracle's trunk carries torchvision's attribute names) re-keyed by
    checkpoint.trunk_state_from_torchvision loads into CILRS.visual_encoder completely."""
    from cilrs_mi355 import CILRS, checkpoint
    tv = O.ResNet34Trunk()                                  # torchvision's names incl. fc
    sd = checkpoint.trunk_state_from_torchvision(tv.state_dict())
    m = CILRS(4, 0.0)
    want = {k for k in m.state_dict() if k.startswith("visual_encoder.")}
    assert set(sd) == want and not any(k.startswith("visual_encoder.9") for k in sd)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert all(not k.startswith("visual_encoder.") for k in res.missing_keys)
    assert torch.equal(m.state_dict()["visual_encoder.5.0.downsample.0.weight"],
                       tv.state_dict()["layer2.0.downsample.0.weight"])
    with pytest.raises(KeyError):
        checkpoint.trunk_state_from_torchvision({"stem.weight": torch.zeros(1)})


def test_steplr_matches_torch_steplr_for_20_epochs():
    """Trainer.scheduler_step's formula against torch.optim.lr_scheduler.StepLR(8, 0.5), the
    reference's scheduler (notebook/notebook.ipynb:535-536), stepped once per epoch (nb:604) for
    20 epochs: the decays at epochs 8 and 16 included."""
    import torch
    from cilrs_mi355.train import CONFIG_A, CONFIG_B, TrainConfig, steplr
    for cfg in (CONFIG_A, CONFIG_B, TrainConfig(lr=3e-4, lr_step_size=3, lr_gamma=0.7)):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([p], lr=cfg.lr)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.lr_step_size, gamma=cfg.lr_gamma)
        assert steplr(cfg, 0) == cfg.lr
        for epoch in range(1, 21):
            opt.step()
            sched.step()
            want = opt.param_groups[0]["lr"]
            got = steplr(cfg, epoch)
            assert abs(got - want) <= 1e-15 + 1e-12 * want, (cfg.name, epoch, got, want)
            if cfg.lr_gamma == 0.5:
                assert got == want                      # powers of two: exact
        if cfg.lr_step_size == 8:
            assert steplr(cfg, 7) == cfg.lr and steplr(cfg, 8) == cfg.lr * 0.5
            assert steplr(cfg, 15) == cfg.lr * 0.5 and steplr(cfg, 16) == cfg.lr * 0.25
