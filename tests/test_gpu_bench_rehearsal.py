"""bench.py's N > 1 loop, rehearsed on the one-GPU box (the loop had never executed).

The driver launches `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` on an 8-GPU node.  RCCL
puts no two ranks on one device, so here every rank renders its tile shard on device 0 and the launch's frames are
gathered by the caller-collective pair of the C-ABI -- rp_frames_pack, a gloo all-gather of the packed blocks,
rp_frames_unpack (RP_BENCH_REHEARSAL=gloo) -- instead of librp's RCCL all-gather.  Everything else is the N-rank loop
itself: the gloo bootstrap, balanced shards, three launches in flight on their own streams and workspaces, the barriers
and the max-over-ranks time, the summed counters, rank 0's single JSON line -- and the frames it assembles, which must
equal the one-GPU run's bit for bit (per-unit seeding; RP_BENCH_DUMP saves the timed run's last launch).
The one-GPU run is a plain one (no --full) with --dump-outputs: test_bench_plain_run_and_dump checks its line and files.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


ARGS = ["--steps", "4", "--warmup", "2", "--spp", "40", "--samples-per-stream", "32", "--no-cpu-baseline"]


@pytest.fixture(scope="module")
def one_gpu_run(tmp_path_factory):
    """The same command on one GPU (no rehearsal), a plain run with --dump-outputs: (its timed run's last launch,
    assembled; its JSON line; the --dump-outputs directory)."""
    d = tmp_path_factory.mktemp("n1")
    out = str(d / "frames.npy")
    r = subprocess.run([sys.executable, "bench.py", *ARGS, "--dump-outputs", str(d / "outputs")], cwd=REPO,
                       env=dict(os.environ, RP_BENCH_DUMP=out), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return np.load(out), json.loads(lines[0]), str(d / "outputs")


@pytest.fixture(scope="module")
def one_gpu_frames(one_gpu_run):
    return one_gpu_run[0]


def test_bench_plain_run_and_dump(gpu, one_gpu_run):
    """A run without --full times its steps and nothing else (no single_frame, no other-contract leg, no cpu_baseline),
    and --dump-outputs writes the last timed frame's outputs: the assembled BGRA8 frame as float32 -- the last frame
    of the last launch, byte for byte -- this rank's linear RGB (a fixed sample of 2^20 of the frame's slots) as float64
    and the launch's counters, under 64 MB in all."""
    frames, d, out = one_gpu_run
    assert d["full"] is False and d["single_frame"] is None and d["cpu_baseline"] is None
    assert "streams_of_32" not in d and "contract_one_stream" not in d and "gpu_over_cpu" not in d
    assert d["steps"] == 4 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"]["launches_all"] == [2, 4]  # the warm-up launch and the timed one: no other launch ran
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert sorted(os.listdir(out)) == ["counters.npy", "frame_bgra.npy", "shard_rgb.npy"]
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64_000_000
    bgra, rgb, ctr = (np.load(os.path.join(out, n + ".npy")) for n in ("frame_bgra", "shard_rgb", "counters"))
    npx = 1920 * 1080
    assert bgra.dtype == np.float32 and bgra.shape == (npx, 4)
    assert np.array_equal(bgra, frames.reshape(-1, npx, 4)[-1].astype(np.float32))
    assert rgb.dtype == np.float64 and rgb.shape == (1 << 20, 3) and np.isfinite(rgb).all()
    assert rgb.max() > 0.0 and len(np.unique(rgb[:, 0])) > 1000
    # the launch's counters: the rays of its 4 frames, no status bit
    assert ctr.dtype == np.float64 and int(ctr[0] / 4) == d["config"]["rays_per_frame"] and ctr[3] == 0
    assert d["dump_outputs"]["arrays"] == {"frame_bgra": [npx, 4], "shard_rgb": [1 << 20, 3], "counters": [len(ctr)]}


@pytest.mark.parametrize("world", [2, 3])
def test_bench_rehearsal(gpu, world, one_gpu_frames, tmp_path):
    dump = str(tmp_path / "frames.npy")
    env = dict(os.environ, RP_BENCH_REHEARSAL="gloo", RP_BENCH_DUMP=dump)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", str(world), *ARGS,
           "--full"]  # single_frame runs with --full only
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]  # rank 0 alone prints: one JSON line
    d = json.loads(lines[0])
    assert d["rehearsal"] is True and "REHEARSAL" in d["config"]["parallelism"]
    assert d["n_gpus"] == world and d["steps"] == 4 and d["value"] > 0 and d["scaling"] == "strong"
    assert d["config"]["samples_per_stream"] == 32 and d["config"]["frames_in_flight"] == 3
    assert d["config"]["shard_map"] == "balanced"
    # the counters the unpack sums over the ranks: every pixel of the 1920 x 1080 frame once per sample
    assert d["config"]["rays_per_frame"] >= 1920 * 1080 * 40
    assert d["single_frame"] and d["single_frame"]["ms_per_frame"] > 0
    # the N-rank frames (balanced shards of 3 launches in flight, packed, gathered, assembled) = the one-GPU frames
    frames = np.load(dump)
    assert frames.shape == one_gpu_frames.shape and frames.size >= 1920 * 1080 * 4
    assert np.array_equal(frames, one_gpu_frames)
