"""The T-table role's window rule in the single-key AES-GCM hybrid kernel
(tlslite-ng_amd/csrc/aes_gcm_bs8.hip octet_job / t_half, WIN), restated on the
oracle's T-table AES like test_window_regrouping.py.

Lane rho of an octet owns the counters 2 + rho + 64 beta + 8 j (batch beta,
block j).  The window constants (win_consts) are kept per window in two
buffers: window beta / 4 sits in buffer (beta / 4) % 2, computed at beta = 0
for the first window and, for every later one, by the batch beta % 4 = 3 of
the window before -- whose block 7 on the lanes rho >= 6 already lies in the
next window and takes those constants.  No batch runs full rounds 1-2, and a
window costs its 15 lookups once."""
import random
import struct

from oracle import pyaead

from test_window_regrouping import Counted, T0, T1, T2, T3, ctr_block_win, record_consts, window_consts


def lane_batches(ks, nonce, rho, betas, t, check):
    """Run the kernel's schedule for lane ``rho`` over batches 0 .. max(betas);
    the blocks of the batches in ``betas`` are checked against the full
    cipher.  Returns (windows computed, blocks run)."""
    cc = record_consts(ks, nonce, (T0, T1, T2, T3))
    buf = [None, None]
    windows = blocks = 0
    for beta in range(max(betas) + 1):
        wnd, cross = beta >> 2, (beta & 3) == 3
        if beta == 0:
            buf[0] = window_consts(ks, cc, 0, t)
            windows += 1
        if cross:
            buf[(wnd + 1) & 1] = window_consts(ks, cc, (wnd + 1) << 8, t)
            windows += 1
        if beta not in betas:
            continue
        c0 = 2 + rho + 64 * beta
        for j in range(8):
            ctr = c0 + 8 * j
            # block 7 of a lane whose first counter has bit 3 set (rho >= 6)
            nxt = cross and j == 7 and ((c0 >> 3) & 1)
            assert bool(nxt) == (ctr >> 8 != wnd), (rho, beta, j)
            W = buf[(wnd + 1) & 1] if nxt else buf[wnd & 1]
            got = ctr_block_win(ks, cc, W, ctr & 255, t)
            blocks += 1
            if check:
                assert got == bytes(pyaead.aes_encrypt(ks, nonce + struct.pack(">I", ctr))), (rho, beta, j)
    return windows, blocks


def test_next_window_for_the_crossing_block():
    rng = random.Random(5)
    plain = (T0, T1, T2, T3)
    for klen in (16, 32):
        ks = pyaead.expand_key(bytes(rng.getrandbits(8) for _ in range(klen)))
        nonce = bytes(rng.getrandbits(8) for _ in range(12))
        # counters 2 .. 2 100, and around 65 535 (batches 1 020 .. 1 027: the
        # rule has no 2^16 limit on this role)
        betas = set(range(0, 33)) | set(range(1020, 1028))
        for rho in range(8):
            lane_batches(ks, nonce, rho, betas, plain, True)


def test_window_rule_lookup_count():
    """15 lookups per window and 5 per block for rounds 1-2: a lane's 16
    batches of a 1 024-block record compute windows 0..4 (beta 0, 3, 7, 11,
    15) and run 128 blocks."""
    ks = pyaead.expand_key(bytes(range(16)))
    nr = ks[0]
    for rho in (0, 6, 7):
        t = tuple(Counted(x) for x in (T0, T1, T2, T3))
        windows, blocks = lane_batches(ks, bytes(12), rho, set(range(16)), t, False)
        assert (windows, blocks) == (5, 128)
        assert sum(x.n for x in t) == 15 * windows + (5 + 16 * (nr - 3)) * blocks
