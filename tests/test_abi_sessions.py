"""CPU checks of the many-session record framing's C ABI
(tg_seal_session_records / tg_open_session_records): the ctypes struct
matches the C layout, the new status has a name, and argument errors are
reported before any HIP call, so they show on a machine without a GPU."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


def test_session_records_struct_layout_matches_c(tmp_path):
    from tlsgpu import _lib
    names = [f[0] for f in _lib.TgSessionRecords._fields_]
    body = "".join('printf("%%zu\\n", offsetof(tg_session_records, %s));\n' % c for c in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlsgpu.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(tg_session_records));\n%sreturn 0;}\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_lib.TgSessionRecords)
    assert len(out) == 1 + len(names)
    for name, off in zip(names, out[1:]):
        assert getattr(_lib.TgSessionRecords, name).offset == off, name
    # every member of the C struct is bound: the fields tile the struct
    # but for alignment padding after the 32-bit members
    assert sum(ctypes.sizeof(t) for _, t in _lib.TgSessionRecords._fields_) + 4 == out[0]


def test_bad_session_status_is_named():
    from tlsgpu import _lib, records
    assert _lib.REC_STATUS[8] == "bad_session"
    assert records.STATUS[8] == "bad_session"


def _filled(_lib, **kw):
    """A struct whose device arrays all look non-NULL (never dereferenced:
    the calls below fail on their arguments first)."""
    r = _lib.TgSessionRecords()
    r.n = 1
    r.version = _lib.TG_TLS13
    r.fixed_iv_len = 12
    r.nsessions = 1
    for name, t in _lib.TgSessionRecords._fields_:
        if t is ctypes.c_void_p and name not in ("seq", "seq_next", "seq_out", "pad_len"):
            setattr(r, name, 0x1000)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@pytest.mark.parametrize("fn", ["tg_seal_session_records", "tg_open_session_records"])
def test_argument_errors_without_a_gpu(fn):
    from tlsgpu import _lib
    lib = _lib.load()
    call = getattr(lib, fn)
    # null key, well-formed struct
    assert call(None, ctypes.byref(_filled(_lib, seq=0x1000)), None) == _lib.TG_EINVAL
    assert b"null" in lib.tg_last_error()
    # null struct
    assert call(None, None, None) == _lib.TG_EINVAL
    assert b"null" in lib.tg_last_error()
    # both / neither of seq and seq_next: reported whatever the key is
    assert call(None, ctypes.byref(_filled(_lib, seq=0x1000, seq_next=0x2000)), None) == _lib.TG_EINVAL
    assert b"seq_next" in lib.tg_last_error() and b"both" in lib.tg_last_error()
    assert call(None, ctypes.byref(_filled(_lib)), None) == _lib.TG_EINVAL
    assert b"seq_next" in lib.tg_last_error() and b"neither" in lib.tg_last_error()
    with pytest.raises(_lib.TlsGpuError):
        _lib.check(call(None, ctypes.byref(_filled(_lib)), None))
    # more records than either mode indexes: refused before anything is launched
    assert call(None, ctypes.byref(_filled(_lib, seq=0x1000, n=2 ** 32 - 1)), None) == _lib.TG_EINVAL
    assert b"2^32 - 2" in lib.tg_last_error()
    assert call(None, ctypes.byref(_filled(_lib, seq_next=0x1000, n=2 ** 40)), None) == _lib.TG_EINVAL
    assert b"2^32 - 2" in lib.tg_last_error()
