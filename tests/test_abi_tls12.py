"""CPU checks of the TLS 1.2 key-setup C ABI (tg_tls12_prf,
tg_cbc_key_create_device, tg_cbc_key_replace_device,
tg_sessions_install_tls12, tg_cbc_sessions_install_tls12): the symbols are
exported, the ctypes struct matches the C layout, and every documented
argument error is reported before any HIP call, so it shows on a machine
without a GPU.  The errors that need a live handle to compare against
(nsessions != nkeys, n > nkeys) are in tests/test_gpu_tls12.py."""
import ctypes
import os
import subprocess

from conftest import ROOT

NEW = ("tg_tls12_prf", "tg_cbc_key_create_device", "tg_cbc_key_replace_device", "tg_sessions_install_tls12",
       "tg_cbc_sessions_install_tls12")


def test_new_symbols_are_exported_and_bound():
    from tlsgpu import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None, name
    assert len(lib.tg_tls12_prf.argtypes) == 11
    assert len(lib.tg_cbc_key_create_device.argtypes) == 8
    assert len(lib.tg_cbc_key_replace_device.argtypes) == 7
    assert len(lib.tg_sessions_install_tls12.argtypes) == 3
    assert len(lib.tg_cbc_sessions_install_tls12.argtypes) == 3


def test_install_struct_layout_matches_c(tmp_path):
    from tlsgpu import _lib
    names = [f[0] for f in _lib.TgTls12Install._fields_]
    body = "".join('printf("%%zu\\n", offsetof(tg_tls12_install, %s));\n' % c for c in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlsgpu.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(tg_tls12_install));\n'
                   'printf("%%d\\n%%d\\n", TG_TLS12_CLIENT_WRITE, TG_TLS12_SERVER_WRITE);\n%sreturn 0;}\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_lib.TgTls12Install)
    assert out[1:3] == [_lib.TG_TLS12_CLIENT_WRITE, _lib.TG_TLS12_SERVER_WRITE]
    assert len(out) == 3 + len(names)
    for name, off in zip(names, out[3:]):
        assert getattr(_lib.TgTls12Install, name).offset == off, name
    # every member of the C struct is bound: the fields tile the struct
    assert sum(ctypes.sizeof(t) for _, t in _lib.TgTls12Install._fields_) == out[0]


def test_prf_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    S, D, O = 0x1000, 0x2000, 0x3000   # device arrays that look non-NULL, never dereferenced

    def err(hashlen=32, secrets=S, secretlen=48, n=1, label=b"key expansion", labellen=13, seeds=D, seedlen=64,
            outlen=104, out=O):
        assert lib.tg_tls12_prf(hashlen, secrets, secretlen, n, label, labellen, seeds, seedlen, outlen, out,
                                None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"secret length must be 1..64" in err(secretlen=0)
    assert b"secret length must be 1..64" in err(secretlen=65)
    assert b"secret length must be 1..128" in err(hashlen=48, secretlen=129)
    assert b"label length" in err(labellen=33, label=bytes(33))
    assert b"seed length" in err(seedlen=129)
    assert b"output length must be 1..256" in err(outlen=0)
    assert b"output length must be 1..256" in err(outlen=257)
    assert b"null label" in err(label=None)
    assert b"null device buffer" in err(secrets=None)
    assert b"null device buffer" in err(out=None)
    assert b"null device buffer" in err(seeds=None)
    # argument errors come before the n == 0 shortcut; a good call of no rows launches nothing
    assert b"output length" in err(n=0, outlen=300)
    assert lib.tg_tls12_prf(32, None, 48, 0, None, 0, None, 0, 32, None, None) == _lib.TG_OK
    assert lib.tg_tls12_prf(48, None, 128, 0, b"x", 1, None, 128, 256, None, None) == _lib.TG_OK


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

    def err(fn, r):
        assert fn(None, ctypes.byref(r) if r is not None else None, None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    for fn, aead in ((lib.tg_sessions_install_tls12, True), (lib.tg_cbc_sessions_install_tls12, False)):
        assert b"null tg_tls12_install" in err(fn, None)
        # a well-formed struct: the key is what is missing
        assert b"null key" in err(fn, _filled(_lib))
        assert b"null key" in err(fn, _filled(_lib, hashlen=48, side=_lib.TG_TLS12_SERVER_WRITE, slot=0x6000,
                                              seq_next=None, fixed_iv_len=12))
        # struct errors are reported whatever the key is
        for h in (0, 20, 64):
            assert b"hashlen must be 32 or 48" in err(fn, _filled(_lib, hashlen=h))
        assert b"side 2" in err(fn, _filled(_lib, side=2))
        for name in ("master_secrets", "client_random", "server_random"):
            assert b"null master_secrets, client_random or server_random" in err(fn, _filled(_lib, **{name: None}))
        if aead:
            for v in (0, 8, 16):
                assert b"fixed_iv_len must be 4 or 12" in err(fn, _filled(_lib, fixed_iv_len=v))
            assert b"null iv_table" in err(fn, _filled(_lib, iv_table=None))
        else:   # CBC ignores both
            assert b"null key" in err(fn, _filled(_lib, fixed_iv_len=0, iv_table=None))


def test_cbc_device_key_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    E, M = 0x1000, 0x2000
    h = ctypes.c_void_p()

    def create(enc=E, keylen=16, mk=M, mackeylen=20, mac=_lib.TG_MAC_SHA1, nkeys=1, out=ctypes.byref(h)):
        assert lib.tg_cbc_key_create_device(enc, keylen, mk, mackeylen, mac, nkeys, out, None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    assert b"null argument" in create(enc=None)
    assert b"null argument" in create(mk=None)
    assert b"null argument" in create(out=None)
    assert b"enc key length must be 16 or 32" in create(keylen=24)
    assert b"unknown mac" in create(mac=0)
    assert b"mac key length must be 1..64" in create(mackeylen=0)
    assert b"mac key length must be 1..64" in create(mackeylen=65, mac=_lib.TG_MAC_SHA256)
    assert b"mac key length must be 1..128" in create(mackeylen=129, mac=_lib.TG_MAC_SHA384)
    assert b"nkeys must be" in create(nkeys=0)
    assert not h.value
    assert lib.tg_cbc_key_replace_device(None, None, E, M, 20, 1, None) == _lib.TG_EINVAL
    assert b"null key" in lib.tg_last_error()
