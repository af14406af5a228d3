"""CPU checks of the many-session AES-CBC + HMAC C ABI (tg_cbc_key_create_table,
tg_cbc_key_info, tg_cbc_key_replace, tg_cbc_seal_session_records,
tg_cbc_open_session_records): the ctypes struct matches the C layout and every
argument error is reported before any HIP call, so it shows on a machine
without a GPU.  (nsessions != nkeys and replace's n > nkeys need a live handle:
tests/test_gpu_cbc_sessions.py.)"""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


def test_cbc_session_struct_layout_matches_c(tmp_path):
    from tlsgpu import _lib
    names = [f[0] for f in _lib.TgCbcSessionRecords._fields_]
    body = "".join('printf("%%zu\\n", offsetof(tg_cbc_session_records, %s));\n' % c for c in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlsgpu.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(tg_cbc_session_records));\n%sreturn 0;}\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_lib.TgCbcSessionRecords)
    assert len(out) == 1 + len(names)
    for name, off in zip(names, out[1:]):
        assert getattr(_lib.TgCbcSessionRecords, name).offset == off, name
    # every member of the C struct is bound: the fields tile the struct
    assert sum(ctypes.sizeof(t) for _, t in _lib.TgCbcSessionRecords._fields_) == out[0]
    assert _lib.REC_STATUS[8] == "bad_session"


def _filled(_lib, **kw):
    """A well-formed counter-mode struct whose device arrays look non-NULL
    (never dereferenced: the calls below fail on their arguments first)."""
    r = _lib.TgCbcSessionRecords()
    r.n, r.version, r.etm, r.nsessions = 4, _lib.TG_TLS12, 0, 3
    r.session, r.seq_next = 0xa000, 0xb000
    r.data, r.data_off, r.data_len, r.ctype = 0x1000, 0x2000, 0x3000, 0x4000
    r.iv, r.wire, r.wire_off, r.wire_len, r.status = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_cbc_session_records_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()

    def err(fn, r):
        assert fn(None, ctypes.byref(r) if r is not None else None, None) == _lib.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for fn in (lib.tg_cbc_seal_session_records, lib.tg_cbc_open_session_records):
        assert b"null tg_cbc_session_records" in err(fn, None)
        # a well-formed struct, in either mode: the key is what is missing
        assert b"null key" in err(fn, _filled(_lib))
        assert b"null key" in err(fn, _filled(_lib, seq=0xc000, seq_next=None, version=_lib.TG_TLS11, etm=1, n=0))
        assert b"null key" in err(fn, _filled(_lib, n=2 ** 32 - 2))
        # the errors of tg_cbc_records, reported whatever the key is
        for v in (0, 0x0300, 0x0301, _lib.TG_TLS13):
            assert b"neither TG_TLS11 nor TG_TLS12" in err(fn, _filled(_lib, version=v))
        assert b"etm must be 0 or 1" in err(fn, _filled(_lib, etm=2))
        # those of tg_session_records
        assert b"exactly one of seq" in err(fn, _filled(_lib, seq=0xc000)) and b"both" in lib.tg_last_error()
        assert b"exactly one of seq" in err(fn, _filled(_lib, seq_next=None)) and b"neither" in lib.tg_last_error()
        for n in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
            assert b"at most 2^32 - 2 records" in err(fn, _filled(_lib, n=n))
        assert b"null session" in err(fn, _filled(_lib, session=None))
    assert b"seal needs iv" in err(lib.tg_cbc_seal_session_records, _filled(_lib, iv=None))
    assert b"null key" in err(lib.tg_cbc_open_session_records, _filled(_lib, iv=None))   # open takes no iv


def test_cbc_table_key_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    keys, mks = bytes(3 * 32), bytes(3 * 128)

    def err(*args):
        assert lib.tg_cbc_key_create_table(*args) == _lib.TG_EINVAL
        assert not h.value
        msg = lib.tg_last_error()
        assert msg
        return msg

    sha1 = _lib.TG_MAC_SHA1
    assert b"null argument" in err(keys, 16, mks, 20, sha1, 3, None)
    assert b"null argument" in err(None, 16, mks, 20, sha1, 3, ctypes.byref(h))
    assert b"null argument" in err(keys, 16, None, 20, sha1, 3, ctypes.byref(h))
    for n in (0, 15, 24, 33):
        assert b"enc key length must be 16 or 32" in err(keys, n, mks, 20, sha1, 3, ctypes.byref(h))
    for m in (0, 4, -1):
        assert b"unknown mac" in err(keys, 16, mks, 20, m, 3, ctypes.byref(h))
    assert b"mac key length must be 1..64" in err(keys, 16, mks, 0, sha1, 3, ctypes.byref(h))
    assert b"mac key length must be 1..64" in err(keys, 16, mks, 65, _lib.TG_MAC_SHA256, 3, ctypes.byref(h))
    assert b"mac key length must be 1..128" in err(keys, 32, mks, 129, _lib.TG_MAC_SHA384, 3, ctypes.byref(h))
    assert b"nkeys must be 1" in err(keys, 16, mks, 20, sha1, 0, ctypes.byref(h))

    # the calls on a handle refuse a missing one
    assert lib.tg_cbc_key_info(None, None, None, None) == _lib.TG_EINVAL and b"null key" in lib.tg_last_error()
    assert lib.tg_cbc_key_replace(None, None, keys, mks, 20, 1, None) == _lib.TG_EINVAL
    assert b"null key" in lib.tg_last_error()
    assert lib.tg_cbc_key_destroy(None) == _lib.TG_OK


def test_python_wrappers_refuse_bad_tables_before_the_library():
    import tlsgpu
    with pytest.raises(ValueError):
        tlsgpu.CbcKey.table([bytes(16)], [bytes(20)], "md5")
    with pytest.raises(ValueError):
        tlsgpu.CbcKey.table([bytes(16), bytes(32)], [bytes(20), bytes(20)], "sha1")     # two suites
    with pytest.raises(ValueError):
        tlsgpu.CbcKey.table([bytes(16), bytes(16)], [bytes(20)], "sha1")
    with pytest.raises(ValueError):
        tlsgpu.CbcKey.table([], [], "sha1")
    with pytest.raises(TypeError):
        tlsgpu.CbcSessions(None, tlsgpu.TLS12, 0)
