"""`bench.py --dump-outputs DIR` on the GPU: the arrays the last timed step handed back, written so that two builds can be compared.
Checked here: names, dtype and shapes; `--steps` sets the number of timed steps (the host-buffer leg of `--full` runs warmup + steps
iterations from the seeds in one call and must end in the timed job's tokens); the dumped arrays agree with each other (every
written-back draw is the token the chain holds, every draw has a finite logit); a second run with the same arguments writes the same
bytes; and so does a plain run, whose line carries no leg of `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS, LENGTH, P, VOCAB = 16, 64, 6, 33


def _bench(dump_dir, steps, warmup, full=True):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    legs = ["--full", "--no-cpu-baseline", "--no-strict", "--no-fp16", "--no-msa", "--no-roofline"] if full else []
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--layers", "2", "--chains", str(CHAINS), "--length", str(LENGTH), *legs, "--dump-outputs", str(dump_dir)],
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return out, {f[:-4]: np.load(os.path.join(dump_dir, f)) for f in sorted(os.listdir(dump_dir))}


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    out, a = _bench(tmp_path / "a", steps=3, warmup=1)
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["host_buffer_entry"]["steps"] == 4 and out["host_buffer_entry"]["equals_device_pointer_job"] is True
    shapes = {"tokens": (CHAINS, LENGTH + 2), "last_step_logits": (CHAINS, P, VOCAB), "last_step_sampled_tokens": (CHAINS, P)}
    assert {k: v.shape for k, v in a.items()} == shapes and all(v.dtype == np.float32 for v in a.values())
    assert out["dumped_outputs"]["float32_arrays"] == {k: list(v) for k, v in shapes.items()}
    tok, lg, st = a["tokens"], a["last_step_logits"], a["last_step_sampled_tokens"]
    assert np.isfinite(lg).all() and lg.std() > 0
    assert (st >= 4).all() and (st <= 23).all() and (st == np.round(st)).all()
    # the last step wrote its P draws into P distinct positions of each chain: every drawn residue is in the final row at least as often
    for c in range(CHAINS):
        want = np.bincount(st[c].astype(int), minlength=VOCAB)
        have = np.bincount(tok[c, 1:-1].astype(int), minlength=VOCAB)
        assert (have >= want).all()
    # the same arguments are the same result, byte for byte
    _, a2 = _bench(tmp_path / "a2", steps=3, warmup=1)
    for k in a:
        assert a[k].tobytes() == a2[k].tobytes(), k
    # a plain run (no --full) times the same steps and dumps the same bytes, and runs no leg beside them
    plain, a3 = _bench(tmp_path / "a3", steps=3, warmup=1, full=False)
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert set(out) - set(plain) == {"host_buffer_entry"} and set(plain) <= set(out)
    for k in a:
        assert a[k].tobytes() == a3[k].tobytes(), k
