"""CPU check of the bitsliced cipher's 256-counter window path (csrc/aes_bs8.h:
v_word, win_words, a_plane, win_sel7, win_rounds, rounds_from) that the
single-key AES-GCM hybrid kernel's bitsliced waves run: compiled with g++
against the C oracle's AES (rijndael.py:922-1038 restated) for AES-128/256,
plain and folded key planes, every lane offset and every batch with counters
below 2^16 in the kernel's own buffer schedule (the batches that cross into
the next window included), then the full-round fallback at and above 2^16
(tests/native/bs8_win_check.cpp).  The same program is built a second time
with AddressSanitizer and UBSan and run stand-alone.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(
        ["g++", "-O2", "-Wall", "-Wno-unknown-pragmas"] + extra + [
            "-I", os.path.join(ROOT, "tlslite-ng_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
            "-o", exe, os.path.join(ROOT, "tests", "native", "bs8_win_check.cpp"),
            "-x", "c", os.path.join(ROOT, "oracle", "aead_oracle.c"), "-lpthread"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_bs8_window_path_matches_encrypt_and_oracle(tmp_path, sanitize):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    out = _build_and_run(tmp_path, "bs8_win_check_san" if sanitize else "bs8_win_check", extra)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("NR=")]
    assert len(lines) == 4 and all(ln.endswith("bad=0") for ln in lines), out.stdout
    assert any("NR=10 fold=1" in ln for ln in lines) and any("NR=14 fold=0" in ln for ln in lines)
    # 8 rho x (1 023 window batches + 7 fallback batches) x 8 blocks; rho 6 and
    # 7 cross into the next window in the 255 batches beta % 4 = 3, beta <= 1 019
    assert all("blocks=65920 crossing_batches=510" in ln for ln in lines), out.stdout
