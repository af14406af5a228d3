"""CPU check of the device's MD5 (csrc/md5.h), built for the host with g++ and
run as a stand-alone program (tests/native/md5_check.cpp): the RFC 1321
appendix A.5 suite, the RFC 2202 HMAC-MD5 cases whose key fits one block (the
only keys the TLS 1.0 / 1.1 PRF of tls10.hip hands it), and messages either
side of the padding boundaries -- 55 / 56 bytes (one block, two) and 119 / 120
(two, three) -- with hashlib's digests.  The program is built a second time
with AddressSanitizer and UBSan and run directly."""
import hashlib
import hmac
import os
import subprocess

from conftest import ROOT
from vectors import detbytes

RFC1321 = [(b"", "d41d8cd98f00b204e9800998ecf8427e"),
           (b"a", "0cc175b9c0f1b6a831c399e269772661"),
           (b"abc", "900150983cd24fb0d6963f7d28e17f72"),
           (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
           (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
           (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
           (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a")]
# RFC 2202 section 2, cases 1-5 (6 and 7 have 80-byte keys, hashed first: out of scope here)
RFC2202 = [(b"\x0b" * 16, b"Hi There", "9294727a3638bb1c13f48ef8158bfc9d"),
           (b"Jefe", b"what do ya want for nothing?", "750c783e6ab0b503eaa86e310a5db738"),
           (b"\xaa" * 16, b"\xdd" * 50, "56be34521d144c88dbb8c733f0e8b3f6"),
           (bytes(range(1, 26)), b"\xcd" * 50, "697eaf0aca3a3aea3a75164746ffaa79"),
           (b"\x0c" * 16, b"Test With Truncation", "56461ef2342edc00f9bab995690efd4c")]
BOUNDARY = [54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 128, 183, 184]


def _hex(b):
    return b.hex() or "-"


def _lines():
    lines = []
    for msg, want in RFC1321:
        assert hashlib.md5(msg).hexdigest() == want
        lines.append("md5 %s %s" % (_hex(msg), want))
    for key, msg, want in RFC2202:
        assert hmac.new(key, msg, hashlib.md5).hexdigest() == want
        lines.append("hmac %s %s %s" % (key.hex(), _hex(msg), want))
    for n in BOUNDARY:
        msg = bytes(detbytes("md5-host-%d" % n, n))
        lines.append("md5 %s %s" % (_hex(msg), hashlib.md5(msg).hexdigest()))
        # behind a key block the same boundaries sit 64 bytes further on
        for keylen in (1, 24, 64):
            key = bytes(detbytes("md5-host-key-%d-%d" % (n, keylen), keylen))
            lines.append("hmac %s %s %s" % (key.hex(), _hex(msg), hmac.new(key, msg, hashlib.md5).hexdigest()))
    return lines


def _run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"] +
                          extra + ["-I", os.path.join(ROOT, "tlslite-ng_amd", "csrc"), "-o", exe,
                                   os.path.join(ROOT, "tests", "native", "md5_check.cpp")])
    lines = _lines()
    path = tmp_path / "md5_cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "CASES n=%d bad=0" % len(lines) in out.stdout and out.stdout.strip().endswith("OK")


def test_device_md5_on_the_host(tmp_path):
    assert len(_lines()) == 7 + 5 + 4 * len(BOUNDARY)
    _run(tmp_path, "md5_check", [])


def test_device_md5_under_sanitizers(tmp_path):
    _run(tmp_path, "md5_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
