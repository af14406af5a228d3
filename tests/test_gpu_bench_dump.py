"""bench.py --dump-outputs: a plain headline run (no --full) writes what its
last timed step computed -- per AEAD the sampled sealed records, the plaintext
opened back for them and open's status -- as float32 .npy files.  One small
run (300 records of 1 000 bytes: more records than the 128 sampled, a length
that is no multiple of the AES block or the 128-byte stride) checked against
the C oracle and against the seeded inputs regenerated here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L = 300, 1000


def test_plain_run_dumps_last_step(tmp_path):
    import bench
    from oracle import oracle
    from vectors import tls13_aad, tls13_nonce
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--records", str(N), "--len", str(L),
                        "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    # a plain run: the timed steps and nothing that takes runs of its own
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["full"] is False and line["verified"] is None and "cpu_baseline" not in line
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value = payload of the 2 steps x 4 launches over the 2 timed steps; the
    # line rounds ms_per_step to 1 us, 2.5 % of a 20 us step, and value to 0.01
    assert line["ms_per_step"] >= 0.02
    assert line["value"] == pytest.approx(4 * N * L / (line["ms_per_step"] / 1e3) / 2 ** 30, rel=0.03, abs=0.01)

    idx = np.load(out / "record_index.npy")
    assert idx.dtype == np.float64
    assert np.array_equal(idx, bench.dump_pick(N, bench.DUMP_RECORDS))
    assert idx[0] == 0 and idx[-1] == N - 1 and np.all(np.diff(idx) > 0) and 120 <= len(idx) <= 128
    files = sorted(os.listdir(out))
    assert files == sorted(["record_index.npy"] + ["%s_%s.npy" % (a, w) for a in
                                                   ("aes128gcm", "chacha20-poly1305")
                                                   for w in ("sealed", "opened", "status")])
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10 ** 6

    # the inputs are seeded: the same bytes here as in the bench's process
    g = torch.Generator(device="cuda").manual_seed(0x7715)
    inp = torch.randint(0, 256, (N * L,), dtype=torch.uint8, device="cuda", generator=g)
    want_pt = inp.view(N, L).cpu().numpy()[idx.astype(np.int64)]
    iv, keys = bench.headline_keys(torch)
    aad = bytes(tls13_aad(L))
    for alg, seal in (("aes128gcm", oracle.gcm_seal), ("chacha20-poly1305", oracle.chacha_seal)):
        sealed = np.load(out / ("%s_sealed.npy" % alg))
        opened = np.load(out / ("%s_opened.npy" % alg))
        status = np.load(out / ("%s_status.npy" % alg))
        assert sealed.dtype == opened.dtype == status.dtype == np.float32
        assert sealed.shape == (len(idx), L + 16) and opened.shape == (len(idx), L)
        assert status.shape == (N,) and np.all(status == 1.0)
        assert np.array_equal(opened, want_pt.astype(np.float32)), alg
        for j, i in enumerate(idx.astype(np.int64)):
            want = seal(keys[alg], bytes(tls13_nonce(iv, int(i))), want_pt[j].tobytes(), aad)
            assert sealed[j].astype(np.uint8).tobytes() == bytes(want), (alg, int(i))
