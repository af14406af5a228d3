"""CPU checks of the in-place rekey C ABI (tg_key_replace_device /
tg_sessions_rekey): the ctypes struct matches the C layout and argument errors
are reported before any HIP call, so they show on a machine without a GPU.
The errors that need a live handle to compare against (nsessions != nkeys,
n > nkeys) are in tests/test_gpu_rekey.py."""
import ctypes
import os
import subprocess

from conftest import ROOT


def test_rekey_struct_layout_matches_c(tmp_path):
    from tlsgpu import _lib
    names = [f[0] for f in _lib.TgRekey._fields_]
    body = "".join('printf("%%zu\\n", offsetof(tg_rekey, %s));\n' % c for c in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tlsgpu.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(tg_rekey));\n'
                   'printf("%%d\\n%%d\\n", TG_REKEY_INSTALL, TG_REKEY_UPDATE);\n%sreturn 0;}\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_lib.TgRekey)
    assert out[1:3] == [_lib.TG_REKEY_INSTALL, _lib.TG_REKEY_UPDATE]
    assert len(out) == 3 + len(names)
    for name, off in zip(names, out[3:]):
        assert getattr(_lib.TgRekey, name).offset == off, name
    # every member of the C struct is bound: the fields tile the struct
    assert sum(ctypes.sizeof(t) for _, t in _lib.TgRekey._fields_) == out[0]


def _filled(_lib, mode, **kw):
    """A well-formed struct for ``mode`` whose device arrays look non-NULL
    (never dereferenced: the calls below fail on their arguments first)."""
    r = _lib.TgRekey()
    r.n, r.mode, r.hashlen, r.nsessions = 1, mode, 32, 1
    r.iv_table, r.seq_next = 0x1000, 0x2000
    if mode == _lib.TG_REKEY_UPDATE:
        r.secrets = 0x3000
    else:
        r.new_secrets = 0x4000
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_sessions_rekey_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    UPD, INS = _lib.TG_REKEY_UPDATE, _lib.TG_REKEY_INSTALL

    def err(r):
        assert lib.tg_sessions_rekey(None, ctypes.byref(r) if r is not None else None, None) == _lib.TG_EINVAL
        return lib.tg_last_error()

    assert b"null tg_rekey" in err(None)
    # a well-formed struct of either mode: the key is what is missing
    assert b"null key" in err(_filled(_lib, UPD))
    assert b"null key" in err(_filled(_lib, INS))
    assert b"null key" in err(_filled(_lib, INS, secrets=0x3000, seq_next=None, slot=0x5000, hashlen=48))
    # struct errors are reported whatever the key is
    bad_mode = _filled(_lib, UPD)
    bad_mode.mode = 2
    assert b"mode 2" in err(bad_mode)
    for h in (0, 16, 20, 64):
        assert b"hashlen must be 32 or 48" in err(_filled(_lib, UPD, hashlen=h))
    assert b"null iv_table" in err(_filled(_lib, UPD, iv_table=None))
    assert b"null iv_table" in err(_filled(_lib, INS, iv_table=None))
    assert b"UPDATE needs the secrets" in err(_filled(_lib, UPD, secrets=None))
    assert b"UPDATE takes no new_secrets" in err(_filled(_lib, UPD, new_secrets=0x4000))
    assert b"INSTALL needs new_secrets" in err(_filled(_lib, INS, new_secrets=None))


def test_key_replace_argument_errors_without_a_gpu():
    from tlsgpu import _lib
    lib = _lib.load()
    assert lib.tg_key_replace_device(None, None, None, 1, None) == _lib.TG_EINVAL
    assert b"null keys" in lib.tg_last_error()
    assert lib.tg_key_replace_device(None, None, 0x1000, 1, None) == _lib.TG_EINVAL
    assert b"null key" in lib.tg_last_error() and b"keys" not in lib.tg_last_error()
    assert lib.tg_key_replace_device(None, 0x2000, 0x1000, 0, None) == _lib.TG_EINVAL
