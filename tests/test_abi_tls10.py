"""CPU checks of the TLS 1.0 / 1.1 key-setup C ABI (tg_tls10_prf,
tg_cbc_sessions_install_tls11): the symbols are declared, exported and bound,
and every argument error that needs no handle is reported before any HIP call,
so it shows on a machine without a GPU.  The errors that need a live handle to
compare against (nsessions != nkeys, n > nkeys, an HMAC-SHA256 / -SHA384
handle) are in tests/test_gpu_tls10.py: a handle cannot be made without a
device."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ("tg_tls10_prf", "tg_cbc_sessions_install_tls11")


def test_new_symbols_are_declared_exported_and_bound():
    from tlsgpu import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tlsgpu.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None, name
    assert len(lib.tg_tls10_prf.argtypes) == 10
    assert len(lib.tg_cbc_sessions_install_tls11.argtypes) == 3
    # the header no longer says the derivation is missing
    assert "NOT covered" not in header and "has no MD5" not in header


def test_prf_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    S, D, O = 0x1000, 0x2000, 0x3000   # device arrays that look non-NULL, never dereferenced

    def err(secrets=S, secretlen=48, n=1, label=b"key expansion", labellen=13, seeds=D, seedlen=64, outlen=104,
            out=O):
        assert lib.tg_tls10_prf(secrets, secretlen, n, label, labellen, seeds, seedlen, outlen, out,
                                None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    assert b"secret length must be 1..128, got 0" in err(secretlen=0)
    assert b"secret length must be 1..128, got 129" in err(secretlen=129)
    assert b"label length must be at most 32" in err(labellen=33, label=bytes(33))
    assert b"seed length must be at most 128" in err(seedlen=129)
    assert b"output length must be 1..256" in err(outlen=0)
    assert b"output length must be 1..256" in err(outlen=257)
    assert b"null label" in err(label=None)
    assert b"n must be at most 2^31" in err(n=2 ** 31 + 1)
    assert b"null device buffer" in err(secrets=None)
    assert b"null device buffer" in err(out=None)
    assert b"null device buffer" in err(seeds=None)
    # the order is tg_tls12_prf's: lengths, label, n, then the buffers
    assert b"secret length" in err(secretlen=0, labellen=33, outlen=0, secrets=None)
    assert b"label length" in err(labellen=33, label=None, seedlen=129)
    assert b"seed length" in err(seedlen=129, outlen=0)
    assert b"output length" in err(outlen=0, label=None)
    assert b"null label" in err(label=None, n=2 ** 31 + 1, out=None)
    # argument errors come before the n == 0 shortcut; a good call of no rows launches nothing
    assert b"output length" in err(n=0, outlen=300)
    assert lib.tg_tls10_prf(None, 48, 0, None, 0, None, 0, 32, None, None) == _lib.TG_OK
    assert lib.tg_tls10_prf(None, 128, 0, b"x", 1, None, 128, 256, None, None) == _lib.TG_OK
    assert lib.tg_tls10_prf(None, 1, 0, None, 0, None, 0, 1, None, None) == _lib.TG_OK


def _filled(_lib, **kw):
    """A well-formed struct whose device arrays look non-NULL (never
    dereferenced: the calls below fail on their arguments first)."""
    r = _lib.TgTls12Install()
    r.n, r.hashlen, r.side, r.nsessions = 1, 32, _lib.TG_TLS12_CLIENT_WRITE, 1
    r.master_secrets, r.client_random, r.server_random = 0x1000, 0x2000, 0x3000
    r.fixed_iv_len, r.iv_table, r.seq_next = 4, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_install_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    fn = lib.tg_cbc_sessions_install_tls11

    def err(r):
        assert fn(None, ctypes.byref(r) if r is not None else None, None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    assert b"null tg_tls12_install" in err(None)
    # a well-formed struct: the key is what is missing
    assert b"null key" in err(_filled(_lib))
    assert b"null key" in err(_filled(_lib, side=_lib.TG_TLS12_SERVER_WRITE, slot=0x6000, seq_next=None))
    # hashlen, fixed_iv_len and iv_table are ignored, whatever they hold
    for h in (0, 20, 32, 48, 64):
        assert b"null key" in err(_filled(_lib, hashlen=h))
    assert b"null key" in err(_filled(_lib, fixed_iv_len=0, iv_table=None))
    assert b"null key" in err(_filled(_lib, fixed_iv_len=7))
    # struct errors are reported whatever the key is
    assert b"side 2" in err(_filled(_lib, side=2))
    for name in ("master_secrets", "client_random", "server_random"):
        assert b"null master_secrets, client_random or server_random" in err(_filled(_lib, **{name: None}))
    assert b"side 9" in err(_filled(_lib, side=9, master_secrets=None))
