"""The ChaCha20-Poly1305 lane kernel's tile loop with wave-relative addressing
and with the pointer rows (tlslite-ng_amd/csrc/chacha_poly.hip: WaveRel,
tiled_blocks_dma) against the C oracle, byte for byte, at the smallest shapes
that reach each branch of the loop and of the choice between the two.

Every output buffer is poisoned first.  After a call the extents of the
records (L + 16 sealed bytes, L opened bytes) must equal the oracle's and
every other byte of the WHOLE buffer must still be
poison: a store past a record, into a gap or into another wave's rows fails.

Each case runs twice: with the default kernel selection, and with
chacha_variant 5, the lane-per-record kernel with the LDS-DMA tile that the
default takes above 49 152 records -- batches this small otherwise go to the
wave-per-record kernel and would not reach the tile loop at all.

Nonces are TLS 1.3's iv xor seq from seq = 2^40 - 3 on, so that all three
nonce words differ between records and the sequence number carries past
2^40 inside a batch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0x5A
SEQ0 = 2 ** 40 - 3
SELECT = [{}, {"chacha_variant": 5}]
SELECT_IDS = ["default", "lane-dma"]


@pytest.fixture(scope="module")
def env(oracle_mod):
    import torch
    import tlsgpu
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vectors import tls13_aad, tls13_nonce
    rng = np.random.default_rng(11)
    key, iv = rng.bytes(32), rng.bytes(12)
    # one plaintext pool and one oracle result per (record, length): shared by
    # all cases, never modified
    pool = rng.integers(0, 256, 16384 + 2049, dtype=np.uint8)
    cache = {}

    def sealed(i, L, k=key):
        """ct || tag of record i (plaintext pool[i : i + L]) under key k."""
        c = cache.get((i, L, k))
        if c is None:
            c = np.frombuffer(bytes(oracle_mod.chacha_seal(k, bytes(tls13_nonce(iv, SEQ0 + i)), pool[i:i + L].tobytes(),
                                                           bytes(tls13_aad(L)))), np.uint8)
            cache[(i, L, k)] = c
        return c

    class E(object):
        pass
    e = E()
    e.torch, e.tg, e.key, e.iv, e.pool, e.sealed, e.aad = torch, tlsgpu, key, iv, pool, sealed, tls13_aad
    e.obj = tlsgpu.HipCHACHA20_POLY1305(bytearray(key))
    return e


def up(e, a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return e.torch.from_numpy(a.view(signed).copy()).cuda()


def check_extents(e, buf, offs, want, what):
    """Every extent equals ``want[i]``; then, with the extents back at the
    poison, the whole buffer is poison.  (A buffer below 256 MiB is compared
    on the host as one image; the 2 GiB ones stay on the device.)"""
    if buf.numel() < (1 << 28):
        got, img = buf.cpu().numpy(), np.full(buf.numel(), POISON, np.uint8)
        for o, w in zip(offs, want):
            img[int(o):int(o) + len(w)] = w
        if not np.array_equal(got, img):
            p = int(np.flatnonzero(got != img)[0])
            i = int(np.argmin(np.where(np.asarray(offs) <= p, p - np.asarray(offs), 1 << 62)))
            raise AssertionError((what, "first difference at buffer offset", p, "= record", i, "+", p - int(offs[i]),
                                  "of", len(want[i]), "expected", int(img[p]), "got", int(got[p])))
        return
    for i, (o, w) in enumerate(zip(offs, want)):
        got = buf[int(o):int(o) + len(w)].cpu().numpy()
        assert np.array_equal(got, w), (what, "record", i, "first difference at",
                                        int(np.flatnonzero(got != w)[0]) if len(w) else None)
        buf[int(o):int(o) + len(w)] = POISON
    assert bool((buf == POISON).all()), (what, "a byte outside every record's extent was written")


def run(e, lens, in_offs, sealed_offs, select, strided=None, obj=None, key_of=None, key_idx=None,
        skipped=(), tamper=None, sizes=None):
    """Seal and open one batch.  ``strided`` = (in stride, sealed stride):
    fixed strides in the descriptor, else offset arrays.  ``skipped``: records
    whose key index is out of range.  ``tamper``: record whose tag gets a bit
    flipped before the open."""
    torch, tg = e.torch, e.tg
    n = len(lens)
    lens = [int(x) for x in lens]
    in_offs, sealed_offs = np.asarray(in_offs, np.int64), np.asarray(sealed_offs, np.int64)
    in_size = sizes[0] if sizes else int((in_offs + np.asarray(lens)).max()) + 256
    sealed_size = sizes[1] if sizes else int((sealed_offs + np.asarray(lens) + 16).max()) + 256
    fixed = len(set(lens)) == 1
    small = max(in_size, sealed_size) < (1 << 28)

    def place(size, fill, offs, parts):
        """A device buffer of ``fill`` with ``parts[i]`` at ``offs[i]``."""
        if small:
            h = np.full(size, fill, np.uint8)
            for o, w in zip(offs, parts):
                h[int(o):int(o) + len(w)] = w
            return up(e, h)
        d = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
        for o, w in zip(offs, parts):
            d[int(o):int(o) + len(w)] = up(e, w)
        return d
    d_in = place(in_size, 0xA5, in_offs, [e.pool[i:i + L] for i, L in enumerate(lens)])
    d_sealed = torch.full((sealed_size,), POISON, dtype=torch.uint8, device="cuda")
    d_back = torch.full((in_size,), POISON, dtype=torch.uint8, device="cuda")
    d_nonce = torch.zeros(12 * n, dtype=torch.uint8, device="cuda")
    tg.make_nonces(e.iv, SEQ0, n, d_nonce)
    d_aad = up(e, np.frombuffer(b"".join(bytes(e.aad(L)) for L in lens), np.uint8))
    d_lens = None if fixed else up(e, lens, np.uint32)
    d_kidx = None if key_idx is None else up(e, key_idx, np.uint32)
    status = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    if strided:
        assert np.array_equal(in_offs, np.arange(n) * strided[0]) and np.array_equal(sealed_offs, np.arange(n) * strided[1])
        lay_seal = dict(in_stride=strided[0], out_stride=strided[1])
        lay_open = dict(in_stride=strided[1], out_stride=strided[0])
    else:
        d_io, d_so = up(e, in_offs, np.uint64), up(e, sealed_offs, np.uint64)
        lay_seal = dict(in_off=d_io, out_off=d_so)
        lay_open = dict(in_off=d_so, out_off=d_io)
    common = dict(aad=d_aad, aad_stride=5, fixed_aad_len=5, lens=d_lens, fixed_len=lens[0] if fixed else 0,
                  key_idx=d_kidx)
    obj = obj if obj is not None else e.obj
    keyf = key_of if key_of is not None else (lambda i: e.key)
    want = [np.zeros(0, np.uint8) if i in skipped else e.sealed(i, L, keyf(i)) for i, L in enumerate(lens)]
    with tg.options(**select):
        tg.seal_batch(obj, tg.make_batch(n, d_in, d_sealed, d_nonce, **dict(common, **lay_seal)))
        torch.cuda.synchronize()
        check_extents(e, d_sealed, sealed_offs, want, ("seal", select, n, lens[:4]))
        # the open reads what the oracle sealed (a skipped record: anything)
        d_sealed = place(sealed_size, POISON, sealed_offs, want)
        if tamper is not None:
            d_sealed[int(sealed_offs[tamper]) + lens[tamper] + 7] ^= 0x10
        tg.open_batch(obj, tg.make_batch(n, d_sealed, d_back, d_nonce, status=status, **dict(common, **lay_open)))
        torch.cuda.synchronize()
    st = status.cpu().numpy()
    bad = set(skipped) | ({tamper} if tamper is not None else set())
    assert st[:n].tolist() == [0 if i in bad else 1 for i in range(n)] and (st[n:] == 0xEE).all()
    # a rejected or skipped record's L plaintext bytes are zeroed, nothing more
    plain = [np.zeros(L, np.uint8) if i in bad else e.pool[i:i + L] for i, L in enumerate(lens)]
    check_extents(e, d_back, in_offs, plain, ("open", select, n, lens[:4]))


def up16(x, m):
    return (x + m - 1) // m * m


FIXED_L = [0, 1, 63, 64, 65, 128, 129, 192, 320, 16384]   # jmin 0, 1, 2, 3, 5, 256 and the tails


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
@pytest.mark.parametrize("align", [16, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_fixed_length_strided(env, n, align, select):
    for L in FIXED_L:
        s_in, s_out = max(up16(L, align), align), up16(L + 16, align)
        run(env, [L] * n, np.arange(n) * s_in, np.arange(n) * s_out, select, strided=(s_in, s_out))


def ragged(n, seed):
    """Lengths with minimum 64 (one tile block for all) and others up to 1 000."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(64, 1001, n)
    lens[rng.integers(0, n)] = 64
    lens[rng.integers(0, n)] = 1000
    return [int(x) for x in lens]


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
@pytest.mark.parametrize("layout", ["strided", "offsets"])
def test_ragged_lengths_in_one_wave(env, layout, select):
    for n, seed in ((64, 1), (130, 2)):
        lens = ragged(n, seed)
        if layout == "strided":
            run(env, lens, np.arange(n) * 1008, np.arange(n) * 1024, select, strided=(1008, 1024))
        else:   # packed at 16-byte aligned offsets: the pointer rows
            io = np.concatenate([[0], np.cumsum([up16(L, 16) for L in lens])[:-1]])
            so = np.concatenate([[0], np.cumsum([up16(L + 16, 16) for L in lens])[:-1]])
            run(env, lens, io, so, select)


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
def test_order_permutation(env, select):
    """The kernel's ``order`` array comes from the planner (dispatch.hip), which
    sorts ragged batches of at least 2 049 records longest first and none
    smaller.  So: a 130-record batch whose records lie permuted in their
    buffers (record i at slot perm[i], offset arrays), and the smallest
    batch the planner orders -- 2 049 records on fixed strides, where the
    order array alone keeps the wave off the wave-relative path."""
    n = 130
    perm = np.random.default_rng(3).permutation(n)
    run(env, ragged(n, 4), perm * 1008, perm * 1024, select)
    n = 2049
    run(env, ragged(n, 7), np.arange(n) * 1008, np.arange(n) * 1024, select, strided=(1008, 1024))


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
def test_unaligned_records(env, select):
    """Offsets = 5 mod 16, as behind a record header: no tile, full_blocks only."""
    n = 65
    for lens in ([320] * n, ragged(n, 5)):
        run(env, lens, np.arange(n) * 1040 + 5, np.arange(n) * 1056 + 5, select)


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
def test_span_too_large_for_wave_relative_addressing(env, select):
    """n = 65, L = 192, strides 2^25: a wave's 64 slots span 2^31 bytes."""
    n, s = 65, 1 << 25
    size = n * s
    run(env, [192] * n, np.arange(n) * s, np.arange(n) * s, select, strided=(s, s), sizes=(size, size))


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
def test_key_table_with_a_key_index_out_of_range(env, select):
    rng = np.random.default_rng(6)
    keys = [rng.bytes(32) for _ in range(3)]
    table = env.tg.KeyTable("chacha20-poly1305", keys)
    n, L = 65, 192
    kidx = [int(x) for x in rng.integers(0, 3, n)]
    kidx[17] = 3
    run(env, [L] * n, np.arange(n) * 192, np.arange(n) * 208, select, strided=(192, 208), obj=table,
        key_of=lambda i: keys[kidx[i]], key_idx=kidx, skipped=(17,))


@pytest.mark.parametrize("select", SELECT, ids=SELECT_IDS)
def test_one_tampered_record(env, select):
    n, L = 65, 320
    run(env, [L] * n, np.arange(n) * 320, np.arange(n) * 336, select, strided=(320, 336), tamper=40)
