"""CPU checks of the AES-CBC + HMAC C ABI (tg_cbc_key_create,
tg_cbc_seal_records, tg_cbc_open_records): the ctypes struct matches the C
layout, the new constants agree with the header, and every argument error is
reported before any HIP call, so it shows on a machine without a GPU."""
import ctypes
import os
import subprocess

from conftest import ROOT

CONSTS = ["TG_TLS11", "TG_MAC_SHA1", "TG_MAC_SHA256", "TG_MAC_SHA384", "TG_REC_DECRYPT_FAILED"]


def test_cbc_struct_layout_and_constants_match_c(tmp_path):
    from tlsgpu import _lib
    names = [f[0] for f in _lib.TgCbcRecords._fields_]
    body = "".join('printf("%%zu\\n", offsetof(tg_cbc_records, %s));\n' % c for c in names)
    consts = "".join('printf("%%d\\n", %s);\n' % c for c in CONSTS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlsgpu.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(tg_cbc_records));\n%s%sreturn 0;}\n' % (consts, body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_lib.TgCbcRecords)
    assert out[1:1 + len(CONSTS)] == [getattr(_lib, c) for c in CONSTS] == [0x0302, 1, 2, 3, 9]
    assert len(out) == 1 + len(CONSTS) + len(names)
    for name, off in zip(names, out[1 + len(CONSTS):]):
        assert getattr(_lib.TgCbcRecords, name).offset == off, name
    # every member of the C struct is bound: the fields tile the struct
    assert sum(ctypes.sizeof(t) for _, t in _lib.TgCbcRecords._fields_) == out[0]
    assert _lib.REC_STATUS[_lib.TG_REC_DECRYPT_FAILED] == "decryption_failed"
    from tlsgpu import records
    assert records.TLS11 == 0x0302


def _filled(_lib, **kw):
    """A well-formed struct whose device arrays look non-NULL (never
    dereferenced: the calls below fail on their arguments first)."""
    r = _lib.TgCbcRecords()
    r.n, r.version, r.etm, r.seq0 = 4, _lib.TG_TLS12, 0, 7
    r.data, r.data_off, r.data_len, r.ctype = 0x1000, 0x2000, 0x3000, 0x4000
    r.iv, r.wire, r.wire_off, r.wire_len, r.status = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_cbc_records_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()

    def err(fn, r):
        assert fn(None, ctypes.byref(r) if r is not None else None, None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    for fn in (lib.tg_cbc_seal_records, lib.tg_cbc_open_records):
        assert b"null tg_cbc_records" in err(fn, None)
        # a well-formed struct: the key is what is missing
        assert b"null key" in err(fn, _filled(_lib))
        assert b"null key" in err(fn, _filled(_lib, version=_lib.TG_TLS11, etm=1, n=0))
        # struct errors are reported whatever the key is
        for v in (0, 0x0300, 0x0301, _lib.TG_TLS13):
            assert b"neither TG_TLS11 nor TG_TLS12" in err(fn, _filled(_lib, version=v))
        assert b"etm must be 0 or 1" in err(fn, _filled(_lib, etm=2))
    assert b"seal needs iv" in err(lib.tg_cbc_seal_records, _filled(_lib, iv=None))
    assert b"null key" in err(lib.tg_cbc_open_records, _filled(_lib, iv=None))   # open takes no iv


def test_cbc_key_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    key32, mk = bytes(32), bytes(128)

    def err(*args):
        assert lib.tg_cbc_key_create(*args) == _lib.TG_EINVAL
        assert not h.value
        return lib.tg_last_error()

    assert b"null argument" in err(key32, 16, mk, 20, _lib.TG_MAC_SHA1, None)
    assert b"null argument" in err(None, 16, mk, 20, _lib.TG_MAC_SHA1, ctypes.byref(h))
    assert b"null argument" in err(key32, 16, None, 20, _lib.TG_MAC_SHA1, ctypes.byref(h))
    for n in (0, 15, 24, 33):
        assert b"enc key length must be 16 or 32" in err(key32, n, mk, 20, _lib.TG_MAC_SHA1, ctypes.byref(h))
    for m in (0, 4, -1):
        assert b"unknown mac" in err(key32, 16, mk, 20, m, ctypes.byref(h))
    assert b"mac key length must be 1..64" in err(key32, 16, mk, 0, _lib.TG_MAC_SHA1, ctypes.byref(h))
    assert b"mac key length must be 1..64" in err(key32, 16, mk, 65, _lib.TG_MAC_SHA256, ctypes.byref(h))
    assert b"mac key length must be 1..128" in err(key32, 32, mk, 129, _lib.TG_MAC_SHA384, ctypes.byref(h))
    assert lib.tg_cbc_key_destroy(None) == _lib.TG_OK


def test_python_wrapper_rejects_an_unknown_mac():
    import pytest
    import tlsgpu
    with pytest.raises(ValueError):
        tlsgpu.CbcKey(bytes(16), bytes(20), "md5")
    assert tlsgpu.cbc.MACS == {"sha1": 1, "sha256": 2, "sha384": 3}
