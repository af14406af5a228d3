"""CPU checks of the TLS 1.3 key-schedule C ABI (tg_hkdf_extract,
tg_hkdf_expand_label_rows, tg_tls13_finished, tg_tls13_handshake_secrets,
tg_tls13_application_secrets): the symbols are exported and bound, and every
documented argument error is reported before any HIP call, so it shows on a
machine without a GPU; n == 0 is TG_OK with nothing launched."""
import ctypes

NEW = {"tg_hkdf_extract": 7, "tg_hkdf_expand_label_rows": 10, "tg_tls13_finished": 6,
       "tg_tls13_handshake_secrets": 10, "tg_tls13_application_secrets": 9}
# device arrays that look non-NULL and far apart, never dereferenced
A, B, C, D, E, G = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def _lib():
    from tlsgpu import _lib
    return _lib, _lib.load()


def test_new_symbols_are_exported_and_bound():
    _l, lib = _lib()
    for name, nargs in NEW.items():
        assert name in _l.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == nargs, name


def test_extract_argument_errors_without_a_gpu():
    _l, lib = _lib()

    def err(hashlen=32, salts=A, ikm=B, ikmlen=32, n=1, out=C):
        assert lib.tg_hkdf_extract(hashlen, salts, ikm, ikmlen, n, out, None) == _l.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"ikm length must be 1..1024" in err(ikmlen=0)
    assert b"ikm length must be 1..1024" in err(ikmlen=1025)
    assert b"ikm length must be 0 or 32" in err(ikm=None, ikmlen=48)
    assert b"ikm length must be 0 or 48" in err(hashlen=48, ikm=None, ikmlen=32)
    assert b"at most 2^31" in err(n=2 ** 31 + 1)
    assert b"null device buffer" in err(out=None)
    # argument errors come before the n == 0 shortcut; a good call of no rows launches nothing
    assert b"ikm length" in err(n=0, ikmlen=2000)
    for args in ((32, None, None, 0, 0, None), (48, None, None, 48, 0, None), (32, A, B, 1024, 0, None)):
        assert lib.tg_hkdf_extract(*args, None) == _l.TG_OK


def test_expand_label_rows_argument_errors_without_a_gpu():
    _l, lib = _lib()

    def err(hashlen=32, secrets=A, n=1, label=b"c hs traffic", labellen=12, contexts=B, ctxlen=32, outlen=32, out=C):
        assert lib.tg_hkdf_expand_label_rows(hashlen, secrets, n, label, labellen, contexts, ctxlen, outlen, out,
                                             None) == _l.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"label length must be at most 32" in err(labellen=33, label=bytes(33))
    assert b"context length must be at most 64" in err(ctxlen=65)
    assert b"output length must be 1..32" in err(outlen=0)
    assert b"output length must be 1..32" in err(outlen=33)
    assert b"output length must be 1..48" in err(hashlen=48, outlen=49)
    assert b"null label" in err(label=None)
    assert b"context length must be 0 or 32" in err(contexts=None, ctxlen=48)
    assert b"context length must be 0 or 48" in err(hashlen=48, contexts=None, ctxlen=32, outlen=48)
    assert b"at most 2^31" in err(n=2 ** 31 + 1)
    assert b"null device buffer" in err(secrets=None)
    assert b"null device buffer" in err(out=None)
    assert b"output length" in err(n=0, outlen=49)
    for args in ((32, None, 0, None, 0, None, 0, 32, None), (48, None, 0, b"x" * 32, 32, None, 48, 1, None),
                 (32, A, 0, b"resumption", 10, B, 64, 32, C)):
        assert lib.tg_hkdf_expand_label_rows(*args, None) == _l.TG_OK


def test_finished_argument_errors_without_a_gpu():
    _l, lib = _lib()

    def err(hashlen=32, secrets=A, hashes=B, n=1, out=C):
        assert lib.tg_tls13_finished(hashlen, secrets, hashes, n, out, None) == _l.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"at most 2^31" in err(n=2 ** 31 + 1)
    for name in ("secrets", "hashes", "out"):
        assert b"null device buffer" in err(**{name: None})
    assert b"hash length" in err(n=0, hashlen=20)
    assert lib.tg_tls13_finished(48, None, None, 0, None, None) == _l.TG_OK


def test_handshake_secrets_argument_errors_without_a_gpu():
    _l, lib = _lib()

    def err(hashlen=32, psk=None, shared=A, sharedlen=32, hello=B, n=1, hs=C, c=D, s=E):
        assert lib.tg_tls13_handshake_secrets(hashlen, psk, shared, sharedlen, hello, n, hs, c, s,
                                              None) == _l.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"shared secret length must be 1..1024" in err(sharedlen=0)
    assert b"shared secret length must be 1..1024" in err(sharedlen=1025)
    assert b"no output" in err(hs=None, c=None, s=None)
    assert b"at most 2^31" in err(n=2 ** 31 + 1)
    assert b"null device buffer" in err(shared=None)
    assert b"null device buffer" in err(hello=None)
    assert b"shared secret length" in err(n=0, sharedlen=0)
    assert lib.tg_tls13_handshake_secrets(32, None, None, 1024, None, 0, C, None, None, None) == _l.TG_OK
    assert lib.tg_tls13_handshake_secrets(48, G, A, 1, B, 0, None, None, E, None) == _l.TG_OK


def test_application_secrets_argument_errors_without_a_gpu():
    _l, lib = _lib()

    def err(hashlen=32, hs=A, fh=B, n=4, master=C, c=D, s=E, e=G):
        assert lib.tg_tls13_application_secrets(hashlen, hs, fh, n, master, c, s, e, None) == _l.TG_EINVAL
        msg = lib.tg_last_error()
        assert msg
        return msg

    for h in (0, 20, 64):
        assert b"hash length must be 32 or 48" in err(hashlen=h)
    assert b"no output" in err(master=None, c=None, s=None, e=None)
    assert b"at most 2^31" in err(n=2 ** 31 + 1)
    assert b"null device buffer" in err(hs=None)
    assert b"null device buffer" in err(fh=None)
    # overlaps: 4 rows of 32 bytes are [p, p + 128)
    assert b"overlaps an input" in err(master=A + 32)          # the handshake secrets, shifted by a row
    assert b"overlaps an input" in err(master=A - 127)
    assert b"overlaps an input" in err(c=A)                    # only master_secret may equal handshake_secret
    assert b"overlaps an input" in err(e=B + 127)
    assert b"overlaps an input" in err(master=B)
    assert b"two outputs overlap" in err(c=D, s=D)
    assert b"two outputs overlap" in err(master=G - 64)
    assert b"two outputs overlap" in err(master=A, c=D, s=D + 127)
    assert b"hash length" in err(n=0, hashlen=0)
    assert lib.tg_tls13_application_secrets(32, None, None, 0, None, None, None, G, None) == _l.TG_OK
    assert lib.tg_tls13_application_secrets(48, A, B, 0, A, None, None, None, None) == _l.TG_OK
