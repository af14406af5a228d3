/*
 * tlsgpu.h -- C ABI of the MI355X TLS record-layer AEAD engine (libtlsgpu.so).
 *
 * This is the drop-in boundary for tlslite-ng's bulk-cipher path.  The
 * reference binds AEAD objects through tlslite/utils/cipherfactory.py
 * (createAESGCM :81-100, createCHACHA20 :144-159) and calls
 * obj.seal(nonce, plaintext, data) / obj.open(nonce, ciphertext, data)
 * (tlslite/utils/aesgcm.py:101,126; tlslite/utils/chacha20_poly1305.py:48,68)
 * once per record from tlslite/recordlayer.py:558 (_encryptThenSeal) and
 * :821 (_decryptAndUnseal).  The ctypes objects in tlsgpu/ (see
 * INTEGRATION.md) bind exactly the functions below.
 *
 * Conventions: plain pointers and sizes, no exceptions across the ABI, every
 * function returns an int status (TG_OK = 0, negative = error; tg_open
 * returns 1 = authentic / 0 = rejected).  A key handle is bound to the device
 * current when it was created.  tg_seal / tg_open may be called on one handle
 * from several threads at once (each call takes its own staging slot: copies
 * of an AEAD object share the handle, recordlayer.py:262, :913);
 * tg_key_destroy must not race with calls on the same handle.  Batch entry
 * points take DEVICE pointers and are ordered on the given HIP stream (NULL =
 * the null stream).
 */
#ifndef TLSGPU_H
#define TLSGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define TG_OK 0
#define TG_EINVAL (-22)      /* bad argument (NULL pointer, bad size) */
#define TG_EKEYLEN (-2)      /* key length: AssertionError (aesgcm.py:37-38) /
                                ValueError (chacha20_poly1305.py:21-22) */
#define TG_ENONCE (-3)       /* nonce length != 12: ValueError
                                (aesgcm.py:107-108, chacha20_poly1305.py:53-54) */
#define TG_ENOMEM (-12)
#define TG_EHIP (-5)         /* a HIP runtime call failed; see tg_last_error() */
#define TG_ENODEV (-19)      /* no GPU visible */

/* Algorithms (the reference's cipher .name values). */
#define TG_AES_GCM 0          /* "aes128gcm" (16-byte key) / "aes256gcm" (32) */
#define TG_CHACHA20_POLY1305 1 /* "chacha20-poly1305" (32-byte key) */
#define TG_AES_CCM 2          /* "aes128ccm" / "aes256ccm": 16-byte tag
                                 (aesccm.py:11-155, cipherfactory.py:102-121) */
#define TG_AES_CCM_8 3        /* "aes128ccm_8" / "aes256ccm_8": 8-byte tag
                                 (cipherfactory.py:123-142) */

typedef struct tg_key tg_key;

/* Library / device. */
const char* tg_version(void);
const char* tg_last_error(void);           /* thread-local message of the last error */
int tg_device_count(int* count);
int tg_init(int device);                   /* hipSetDevice for the calling thread */

/* Kernel-selection options (process-wide; tests and measurement -- the
 * engine's own choice is value 0 everywhere).  Each starts from its TLSGPU_*
 * environment variable, read once at first use:
 *   gcm_variant        0 auto, 6 wave per record, 14 bitsliced octet,
 *                      15 hybrid octet, 16 T-table lane per record
 *   gcm_table_variant  0 auto (<= 2048 records, or one length with <= 16 MiB
 *                      in all: wave per record without a plan; else the
 *                      length split), 1 lane, 5 wave per record,
 *                      6 wave per record with 4-bit GHASH tables,
 *                      14 key-grouped octet
 *   kt_split           key-table length split in bytes (0 = 2048)
 *   kt_lpr             key-table long records: lanes per record of the
 *                      key-grouped bitsliced kernel (8 / 16 / 32 / 64; 0 =
 *                      32), -1 = the wave-per-record T-table kernel
 *   kt_hybrid, kt_t    key-table long records at 32 lanes per record: 0 =
 *                      the persistent T-table + bitsliced kernel, -1 = the
 *                      bitsliced key-grouped kernel; its T-table waves (0 =
 *                      7 of 11, at most 11)
 *   kt_overlap         key tables: the short records' lane kernel on a
 *                      helper stream of the caller's stream beside the long
 *                      records' kernel (0 = on, -1 = both on the caller's
 *                      stream)
 *   chacha_variant     0 auto, 3 wave per record, 4 lane per record with
 *                      the register-staged tile, 5 lane per record with the
 *                      LDS-DMA tile (auto's choice for large batches),
 *                      6 eight lanes per record (octets, single key)
 *   ccm_variant        0 auto, 1 lane full rounds, 2 wave, 3 lane, 4 hybrid
 *                      (bitsliced keystream + T-table MAC waves, single key),
 *                      5 / 6 / 7 / 8 lane with the payload 1 / 2 / 4 / 8
 *                      blocks ahead (auto's single-key choice: 4)
 *   ccm_hy_t           T-table waves of the CCM hybrid (0 = 4 of 12, -1 none)
 *   waves_per_record   0 auto, 1 / 4 / 16
 *   no_plan            1 = no length-sorted launch order
 *   stage_copy         1 = per-record calls copy through device memory
 *   hy_t, hy_prio      hybrid AES-GCM kernel: T-table waves (0 = auto: 10
 *                      of 16, -1 = none; more than the workgroup's waves
 *                      fails the launch with TG_EINVAL), 1 = T-table waves
 *                      at raised priority
 *   hy_threads         hybrid AES-GCM workgroup: 0 = 1024, or 768
 * An unknown name is TG_EINVAL; a variant a launcher does not know makes
 * its launches fail with TG_EINVAL. */
int tg_set_option(const char* name, int value);
int tg_get_option(const char* name, int* value);

/* Keys -- replaces python_aesgcm.new (python_aesgcm.py:10-11) and
 * python_chacha20_poly1305.new (python_chacha20_poly1305.py:9-11): expands the
 * AES round keys and the GHASH tables for H = E_K(0) (aesgcm.py:27-57) on the
 * host and uploads them once.  nkeys > 1 builds a key table indexed by
 * tg_batch.key_idx (many sessions in one batch). */
int tg_key_create(int alg, const uint8_t* keys, size_t keylen, size_t nkeys,
                  tg_key** out);
/* tg_key_destroy waits for the device (batches on any stream may still read
 * the key), then scrubs and frees the key material. */
int tg_key_destroy(tg_key* k);
int tg_key_info(const tg_key* k, int* alg, size_t* keylen, size_t* nkeys);

/* Tag length of a key's algorithm: 16, or 8 for TG_AES_CCM_8.  Below, "T"
 * is this length. */
int tg_key_taglen(const tg_key* k);
/* Per-record drop-in, HOST buffers (synchronous).
 * tg_seal: out receives ct || tag (len + T bytes) -- AESGCM.seal /
 *   CHACHA20_POLY1305.seal / AESCCM.seal.
 * tg_open: in = ct || tag (inlen bytes); pt receives inlen - T bytes.
 *   Returns 1 when the tag verifies, 0 when the record is rejected (the
 *   reference's None: bad tag, or inlen < T), negative on error.
 *   On rejection pt is zeroed, never left holding unauthenticated bytes. */
int tg_seal(tg_key* k, const uint8_t* nonce, size_t noncelen,
            const uint8_t* aad, size_t aadlen, const uint8_t* pt, size_t len,
            uint8_t* out);
int tg_open(tg_key* k, const uint8_t* nonce, size_t noncelen,
            const uint8_t* aad, size_t aadlen, const uint8_t* in, size_t inlen,
            uint8_t* pt);

/* Batch of records, DEVICE pointers.  Record i:
 *   payload  in  + (in_off  ? in_off[i]  : i * in_stride),  len[i] bytes
 *            (seal: plaintext; open: ciphertext, followed by its T-byte tag)
 *   output   out + (out_off ? out_off[i] : i * out_stride)
 *            (seal: ct || tag, len[i] + T bytes; open: pt, len[i] bytes)
 *   nonce    nonce + 12 * i (12 bytes)
 *   aad      aad + (aad_off ? aad_off[i] : i * aad_stride),
 *            aad_len ? aad_len[i] : fixed_aad_len bytes
 *   key      key table entry key_idx ? key_idx[i] : 0; key_idx[i] must be
 *            below the table's nkeys -- a record with an index out of range
 *            is skipped (never read past the table; open: status[i] = 0
 *            and its plaintext output zeroed, as a rejected record's)
 *   status   open only: status[i] = 1 authentic / 0 rejected (pt zeroed)
 * len == NULL means every record is fixed_len bytes.  Offsets with 16-byte
 * alignment take the vector path; any alignment is accepted.
 * Nothing outside a record's own output extent and status[0..n) is written:
 * a seal extent is len[i] + T bytes (ct || tag), an open extent len[i] bytes
 * (the plaintext, or len[i] zero bytes for a rejected or skipped record; the
 * tag and the rest of a partial last block are never stored behind it), at
 * any alignment of either side.  Inputs (in, nonce, aad and every offset,
 * length and index array) are never written.
 * Records are independent; nothing is ordered between them.  AES-CCM records
 * must be shorter than 2^28 - 32 bytes (the 3-byte CCM counter; TLS records
 * are at most 2^14 + 256). */
typedef struct tg_batch {
    uint64_t n;
    const uint8_t* in;
    const uint64_t* in_off;
    uint64_t in_stride;
    const uint32_t* len;
    uint32_t fixed_len;
    uint32_t fixed_aad_len;
    uint8_t* out;
    const uint64_t* out_off;
    uint64_t out_stride;
    const uint8_t* nonce;
    const uint8_t* aad;
    const uint64_t* aad_off;
    uint64_t aad_stride;
    const uint32_t* aad_len;
    const uint32_t* key_idx;
    uint8_t* status;
} tg_batch;

int tg_seal_batch(tg_key* k, const tg_batch* b, void* stream);
int tg_open_batch(tg_key* k, const tg_batch* b, void* stream);

/* Build per-record 12-byte nonces on the device from a connection's fixed IV
 * and sequence numbers, as RecordLayer._getNonce does (recordlayer.py:522-534):
 *   mode 0 (TLS 1.3 / RFC ChaCha): nonce_i = iv12 xor (0^4 || be64(seq0 + i))
 *   mode 1 (TLS 1.2 AES-GCM / AES-CCM, draft ChaCha):
 *          nonce_i = iv4 || be64(seq0 + i)
 * out: device, 12 * n bytes. */
int tg_make_nonces(int mode, const uint8_t* iv, size_t ivlen, uint64_t seq0,
                   uint64_t n, uint8_t* out, void* stream);

/* TLS record framing on the device -- the callers either side of the AEAD in
 * tlslite/recordlayer.py: _getNonce (:522-534), _encryptThenSeal (:536-565,
 * AAD, TLS 1.2 AES-GCM / AES-CCM explicit nonce), sendRecord (:606-617, TLS 1.3 inner
 * content type + zero padding, 5-byte header), _decryptAndUnseal (:780-824,
 * publicly-invalid checks) and _tls13_de_pad (:863-884).  Record i has
 * sequence number seq0 + i.  All arrays are DEVICE pointers.
 *   seal: fragment data + data_off[i], data_len[i] bytes, content type
 *         ctype[i]; TLS 1.3 appends ctype[i] and pad_len[i] zero bytes IN
 *         PLACE after the fragment (the data buffer needs that much slack),
 *         then writes the whole record (header || [explicit nonce] || ct ||
 *         tag) at wire + wire_off[i] and its size to wire_len[i].
 *   open: wire record (header included) at wire + wire_off[i], wire_len[i]
 *         bytes; plaintext goes to data + data_off[i] (room for the inner
 *         plaintext), its length to data_len[i], the (inner) content type to
 *         ctype[i], and a TG_REC_* code to status[i].
 * For the vector path place records so the payload after the header (and
 * TLS 1.2 AES explicit nonce) is 16-byte aligned.  The tag is T bytes.
 * Nothing outside a record's own extents and entries [0, n) of the result
 * arrays (seal: wire_len; open: data_len, ctype, status) is written:
 *   seal: in wire, the wire_len[i] bytes of the record.  In data, TLS 1.3
 *         writes bytes [data_len[i], data_len[i] + 1 + pad_len[i]) of the
 *         fragment's extent (the content type, then zeros) -- the one write
 *         to an input; a TLS 1.2 seal leaves data as it was.  The data
 *         extent needs no room for the tag.
 *   open: in data, the inner plaintext's bytes: wire_len[i] - 5 - [8] - T
 *         (TLS 1.3: content, type, then the padding's zeros; TLS 1.2: the
 *         content), and nothing behind them.  For TG_REC_BAD_MAC those
 *         bytes are zero; for a record refused before decryption
 *         (TG_REC_TRUNCATED, TG_REC_LENGTH, TG_REC_BAD_TYPE,
 *         TG_REC_BAD_VERSION, TG_REC_OVERFLOW by the header's length) not a
 *         byte of data is written.  wire is never written.
 * The offset arrays, seal's data_len / ctype / pad_len and open's wire_len
 * are never written.
 * Open's checks, in order; the first that fails is the record's status
 * (B = wire_len[i] - 5, E = 8 for TLS 1.2 AES-GCM / AES-CCM, else 0):
 *   1. wire_len[i] < 5, B < E or B - E < T   TG_REC_TRUNCATED
 *   2. B > recv_limit + 2048, or TLS 1.3 and
 *      B > recv_limit + 256                  TG_REC_OVERFLOW (by the header)
 *   3. TLS 1.3: outer type != 23             TG_REC_BAD_TYPE
 *   4. TLS 1.3: version != 0x0303            TG_REC_BAD_VERSION
 *   5. TLS 1.3: header length != B           TG_REC_LENGTH
 *      (TLS 1.2: the header's version and length bytes are not looked at,
 *      its type goes into the AAD)
 *   6. the tag                               TG_REC_BAD_MAC
 *   7. TLS 1.3: inner plaintext > limit + 1  TG_REC_OVERFLOW
 *   8. TLS 1.3: inner plaintext all zero     TG_REC_NO_CONTENT_TYPE
 *   9. content > recv_limit                  TG_REC_OVERFLOW
 * This is the reference's order (RecordSocket.recv, _decryptAndUnseal,
 * recvRecord) but for 1 and 2, which cannot coincide with a header a socket
 * delivers.  So a cut body wins over a wrong header, a bad tag over a
 * refusal after decryption (7-9), the header's overflow over a bad tag.
 * For every status but TG_REC_OK data_len[i] = 0 and ctype[i] = 0.  A record
 * refused after decryption (7-9) has passed the tag: its authentic inner
 * plaintext stays in its data extent; it is not zeroed.
 * wire_len[i] < 5 is not even a header: bytes [0, wire_len[i]) at wire_off[i]
 * are the only ones read, status[i] = TG_REC_TRUNCATED, ctype[i] = 0,
 * data_len[i] = 0 and nothing is written to data.
 * Unprotected TLS 1.3 records are NOT handled here.  With an encrypting read
 * state the reference passes two kinds of record through undecrypted and
 * gives them no sequence number (recvRecord :920-933): outer type 20
 * (ChangeCipherSpec, any body), and outer type 21 with a body under 3 bytes
 * while seqnum == 0 (an alert before the first protected record).  Here they
 * get TG_REC_BAD_TYPE, or TG_REC_TRUNCATED where the body is shorter than the
 * tag, and in a batch they would take a sequence number: the caller takes
 * them out before batching. */
#define TG_TLS12 0x0303
#define TG_TLS13 0x0304
#define TG_REC_OK 0
#define TG_REC_BAD_MAC 1        /* TLSBadRecordMAC (recordlayer.py:822-823) */
#define TG_REC_TRUNCATED 2      /* "Truncated nonce" / "Truncated tag" (:788-789, :797-799) */
#define TG_REC_LENGTH 3         /* "Length mismatch" (:816-817) */
#define TG_REC_BAD_TYPE 4       /* TLSUnexpectedMessage, encrypted non-app-data (:809-812) */
#define TG_REC_BAD_VERSION 5    /* TLSIllegalParameterException (:813-815) */
#define TG_REC_NO_CONTENT_TYPE 6 /* malformed inner plaintext (:880-882) */
#define TG_REC_OVERFLOW 7       /* TLSRecordOverflow: header length over the limit
                                   (RecordSocket.recv :219-222), TLS 1.3 inner
                                   plaintext over limit + 1 (:974-975), plaintext
                                   over limit (:980-981) */

typedef struct tg_records {
    uint64_t n;
    uint32_t version;           /* TG_TLS12 or TG_TLS13 */
    uint32_t fixed_iv_len;      /* 4 (TLS 1.2 AES-GCM / AES-CCM) or 12 */
    uint8_t fixed_iv[12];
    uint32_t recv_limit;        /* open: recv_record_limit (0 = 2^14, recordlayer.py:56) */
    uint64_t seq0;
    uint8_t* data;
    const uint64_t* data_off;
    uint32_t* data_len;
    uint8_t* ctype;
    const uint32_t* pad_len;    /* seal, TLS 1.3 only; NULL = no padding */
    uint8_t* wire;
    const uint64_t* wire_off;
    uint32_t* wire_len;
    uint8_t* status;            /* open */
} tg_records;

int tg_seal_records(tg_key* k, const tg_records* r, void* stream);
int tg_open_records(tg_key* k, const tg_records* r, void* stream);

/* Record framing for MANY sessions in one batch: the pending records of many
 * RecordLayers (one direction each) through one call.  Record i belongs to
 * session s = session[i]; it is sealed / opened under key-table entry s with
 * the fixed IV in row s of iv_table and a per-session sequence number.  The
 * nonce, AAD, header, explicit-nonce, TLS 1.3 inner-plaintext, limit and
 * de-padding rules, and the data / wire arrays, are those of tg_records; one
 * TLS version and one algorithm (the key handle's) per batch.  All arrays
 * are DEVICE pointers.
 *   nsessions  must equal the key handle's nkeys (a single-key handle with
 *              nsessions == 1 is valid).
 *   iv_table   nsessions rows of fixed_iv_len bytes, packed -- the layout
 *              tg_hkdf_expand_label writes for the "iv" label.
 *   Exactly one of seq / seq_next is given (anything else is TG_EINVAL):
 *   seq        explicit mode: record i has sequence number seq[i].
 *   seq_next   counter mode: nsessions counters, one per session (a
 *              RecordLayer's _writeState.seqnum / _readState.seqnum).  Record
 *              i gets seq_next[s] as it was before the call plus the number
 *              of earlier records j < i of this batch with session[j] == s;
 *              after the call seq_next[s] has advanced by the session's
 *              record count (sessions without records are untouched).  The
 *              assignment follows batch order and is deterministic.  On open
 *              every record with session[i] < nsessions consumes a number
 *              whatever its status.  The reference does so for every record
 *              that reaches _decryptAndUnseal (getSeqNumBytes() at its top,
 *              recordlayer.py:782) and differs for two kinds that do not: a
 *              record refused by the header's length (RecordSocket.recv
 *              :219-222, TG_REC_OVERFLOW before decryption) and an
 *              unprotected TLS 1.3 record (see tg_records) consume no number
 *              there.  The first is fatal to its connection either way; the
 *              second must not be in the batch.  The numbers come from a stable sort
 *              of the batch by session (one algorithm, and no kernel with a
 *              private segment, at every n).
 *   seq_out    optional, n entries: the number record i was given, in either
 *              mode (not written for a skipped record).
 * A record with session[i] >= nsessions is skipped: nothing is read past
 * either table and no sequence number is consumed; seal writes nothing to
 * wire and sets wire_len[i] = 0; open sets status[i] = TG_REC_BAD_SESSION,
 * data_len[i] = 0 and ctype[i] = 0 and writes nothing to data.  That test
 * comes before every other; for an in-range record the order of open's
 * checks, the 0 / 0 rule for every refusal, the plaintext left by a refusal
 * after decryption, the wire_len[i] < 5 rule and the exclusion of unprotected
 * TLS 1.3 records are those of tg_records.
 * n is at most 2^32 - 2 in either mode; a larger n is TG_EINVAL before anything
 * is launched.  Two calls that share seq_next must be ordered on one stream. */
#define TG_REC_BAD_SESSION 8    /* session[i] >= nsessions: record skipped */

typedef struct tg_session_records {
    uint64_t n;
    uint32_t version;           /* TG_TLS12 or TG_TLS13, one per batch */
    uint32_t fixed_iv_len;      /* 4 or 12, one per batch: the rule of tg_records */
    uint32_t recv_limit;        /* open: recv_record_limit (0 = 2^14) */
    uint64_t nsessions;
    const uint8_t* iv_table;
    const uint32_t* session;
    const uint64_t* seq;
    uint64_t* seq_next;
    uint64_t* seq_out;
    uint8_t* data;
    const uint64_t* data_off;
    uint32_t* data_len;
    uint8_t* ctype;
    const uint32_t* pad_len;    /* seal, TLS 1.3 only; NULL = no padding */
    uint8_t* wire;
    const uint64_t* wire_off;
    uint32_t* wire_len;
    uint8_t* status;            /* open */
} tg_session_records;

int tg_seal_session_records(tg_key* k, const tg_session_records* r, void* stream);
int tg_open_session_records(tg_key* k, const tg_session_records* r, void* stream);

/* Bulk TLS 1.3 key setup on the device -- the
 * per-session work of RecordLayer.calcTLS1_3PendingState
 * (recordlayer.py:1268-1323) and _calcTLS1_3KeyUpdate (:1325-1350) for many
 * sessions at once, all buffers DEVICE pointers.
 * tg_hkdf_expand_label: out[i] = HKDF-Expand-Label(secrets[i], label,
 *   context, outlen) (cryptomath.py:155-173, HKDF_expand :146-153, HMAC
 *   :128-132) for i < n; hashlen 32 (SHA-256) or 48 (SHA-384) is both the
 *   PRF and the secret size; 1 <= outlen <= hashlen (every record-layer use:
 *   "key", "iv", "traffic upd", "finished").  Secrets at hashlen * i, outputs
 *   at outlen * i.
 * tg_key_create_device: tg_key_create with the keys (nkeys x keylen) already
 *   in device memory: the AES key schedule, H = E_K(0) and the GHASH tables
 *   are built by kernels on `stream` (synchronised before returning), so
 *   derived keys never visit the host. */
int tg_hkdf_expand_label(int hashlen, const uint8_t* secrets, uint64_t n, const uint8_t* label,
                         size_t labellen, const uint8_t* context, size_t ctxlen, size_t outlen,
                         uint8_t* out, void* stream);
int tg_key_create_device(int alg, const uint8_t* keys, size_t keylen, size_t nkeys,
                         tg_key** out, void* stream);

/* Rekeying entries of a LIVE key handle in place: a closed connection's slot
 * taken by a new one, and TLS 1.3 KeyUpdate (RecordLayer._calcTLS1_3KeyUpdate,
 * recordlayer.py:1325-1349, calcTLS1_3KeyUpdate_sender / _reciever
 * :1351-1375).  Both calls are kernels on `stream` and nothing else: no host
 * synchronisation, no table allocation, no key material copied to the host.
 * The handle gives the algorithm and key length; every handle type is covered
 * (AES-GCM tables with their derived arrays, AES-CCM / CCM_8,
 * ChaCha20-Poly1305, and the single-key AES-GCM handle: nkeys == 1, slot 0,
 * all of its GHASH tables and key planes).  All arrays are DEVICE pointers.
 *   slot   n entries, the table rows to rebuild; NULL = rows 0..n-1.  A slot
 *          that is not below nkeys is skipped: nothing of any table is read
 *          or written for it (tg_sessions_rekey: its secret, IV and counter
 *          stay untouched).  The slots of one call must be DISTINCT: with a
 *          duplicate, the row may end up mixing material of both keys.
 *   n == 0 is TG_OK with nothing launched; n > nkeys is TG_EINVAL.  Every
 *   argument error (NULL key / struct / keys / iv_table, bad mode or hashlen,
 *   nsessions != nkeys, UPDATE without secrets or with new_secrets, INSTALL
 *   without new_secrets) is reported before any HIP call.
 * Every byte of a rebuilt row's old material is overwritten (round keys, H,
 * its powers, the key planes and the rotated round keys).
 * ORDERING follows `stream` only.  Batches enqueued on `stream` before the
 * call use the old entries, batches enqueued after it the new ones.  Work on
 * other streams that uses the handle (or iv_table / secrets / seq_next) must
 * be ordered against the call by the caller (events), and the caller must
 * synchronise `stream` before using the host-buffer calls tg_seal / tg_open
 * on the handle, which run on staging streams of their own.
 *
 * tg_key_replace_device: row j of keys (n x keylen bytes) becomes the key of
 *   entry slot[j].
 * tg_sessions_rekey: for each selected slot s (list position j), as
 *   _calcTLS1_3KeyUpdate and calcTLS1_3PendingState (:1291-1316) do:
 *     TG_REKEY_UPDATE   secret' = HKDF-Expand-Label(secrets[s], "traffic upd",
 *                       "", hashlen), written back to secrets[s];
 *     TG_REKEY_INSTALL  secret' = new_secrets[j], copied to secrets[s] when
 *                       the table is given;
 *   then key = Expand-Label(secret', "key", "", keylen) rebuilds entry s (the
 *   raw key exists in registers only), iv_table[s] = Expand-Label(secret',
 *   "iv", "", 12), and seq_next[s] = 0 when seq_next is given (the fresh
 *   ConnectionState's seqnum). */
int tg_key_replace_device(tg_key* k, const uint32_t* slot, const uint8_t* keys,
                          uint64_t n, void* stream);

#define TG_REKEY_INSTALL 0  /* a new connection takes the slot: secret given */
#define TG_REKEY_UPDATE  1  /* TLS 1.3 KeyUpdate: the slot's secret advances */
typedef struct tg_rekey {
    uint64_t n;
    uint32_t mode;
    uint32_t hashlen;           /* 32 (SHA-256) or 48 (SHA-384) */
    uint64_t nsessions;         /* must equal the handle's nkeys */
    const uint32_t* slot;       /* n entries; NULL = 0..n-1 */
    const uint8_t* new_secrets; /* INSTALL: n x hashlen; UPDATE: must be NULL */
    uint8_t* secrets;           /* nsessions x hashlen table.  UPDATE: required,
                                   row advanced in place.  INSTALL: optional,
                                   row overwritten with the new secret */
    uint8_t* iv_table;          /* nsessions x 12, required */
    uint64_t* seq_next;         /* optional: counters of the slots set to 0 */
} tg_rekey;
int tg_sessions_rekey(tg_key* k, const tg_rekey* r, void* stream);

/* TLS 1.2 key setup on the device -- the per-connection work of
 * RecordLayer.calcPendingStates (recordlayer.py:1189-1246) and of calc_key
 * (mathtls.py) for many sessions at once, so a TLS 1.2 session's keys never
 * visit the host either.  TLS 1.0 / 1.1 derivation -- their PRF is
 * P_MD5 xor P_SHA1 (mathtls.py:701-714) -- has the same two steps:
 * tg_tls10_prf and tg_cbc_sessions_install_tls11, below.  (TLS 1.0 RECORDS
 * stay out of scope: their implicit IV chains a connection's records.)
 *
 * tg_tls10_prf: out[i] = PRF(secrets[i], label, seeds[i], outlen) of
 *   mathtls.py:701-714 for i < n, one session per lane:
 *     P_hash(md5, S1, label || seed) xor P_hash(sha1, S2, label || seed)
 *   byte by byte, with S1 the first and S2 the last ceil(secretlen / 2) bytes
 *   of the secret (they share the middle byte of an odd length).  Pointers and
 *   limits are tg_tls12_prf's: secrets, seeds and out are DEVICE pointers, rows
 *   packed, any alignment; label is HOST memory; labellen at most 32, seedlen
 *   at most 128, outlen 1 .. 256, n at most 2^31.  secretlen is 1 .. 128, so
 *   either half is at most one 64-byte block and is never hashed first.  Every
 *   argument error is TG_EINVAL before any HIP call, worded and ordered as
 *   tg_tls12_prf's; n == 0 is TG_OK with nothing launched; nothing but
 *   out[0, n outlen) is written.  It serves TLS 1.0 and 1.1 alike: "master
 *   secret" (seed client_random || server_random), "key expansion", and
 *   "extended master secret", "client finished" / "server finished" (seed =
 *   the 36 bytes MD5(handshake) || SHA1(handshake)).  Kernels on `stream` and
 *   library scratch only (four padded message templates per session, holding
 *   label and seed, never the secret).
 *
 * tg_cbc_sessions_install_tls11: tg_cbc_sessions_install_tls12 for TLS 1.1
 *   connections, with the same struct; hashlen, fixed_iv_len and iv_table are
 *   IGNORED.  For list position j and slot s = slot[j] the key block
 *     PRF(master_secrets[j], "key expansion", server_random[j] ||
 *         client_random[j])
 *   is cut as calcPendingStates cuts it -- client MAC (20 bytes), server MAC,
 *   client key, server key -- and the slices of `side` rebuild row s whole
 *   (forward schedule, the equivalent inverse cipher's schedule, the two
 *   HMAC-SHA1 midstates); seq_next[s] = 0 when seq_next is given; the two
 *   16-byte IV blocks that follow are not derived.  Only what a TLS 1.1 AES
 *   suite can produce is built: the handle's MAC must be TG_MAC_SHA1 (AES-128
 *   or AES-256); an HMAC-SHA256 / -SHA384 handle is TG_EINVAL.  The rest is
 *   tg_cbc_sessions_install_tls12's contract word for word: a slot >= nkeys is
 *   skipped with nothing read or written for it, the slots must be DISTINCT,
 *   ORDERING follows `stream` only, no host synchronisation and no key
 *   material on the host, every byte of a rebuilt row is overwritten, argument
 *   errors (NULL struct / key / master_secrets / client_random /
 *   server_random, bad side, nsessions != nkeys, n > nkeys, n > 2^31, the
 *   handle's MAC) are TG_EINVAL before any HIP call, n == 0 is TG_OK.
 *
 * tg_tls12_prf: out[i] = P_hash(secrets[i], label || seeds[i], outlen)
 *   (mathtls.py:679-698) as PRF_1_2 (hashlen 32, SHA-256) and PRF_1_2_SHA384
 *   (hashlen 48) use it (:716-722), for i < n, one session per lane.  secrets
 *   (n x secretlen), seeds (n x seedlen) and out (n x outlen) are DEVICE
 *   pointers, rows packed, any alignment; label is HOST memory and shared by
 *   all rows.
 *     secretlen  1 .. the hash's block size (64, SHA-384: 128); that covers the
 *                48-byte master and premaster secrets.  A longer secret is
 *                TG_EINVAL: HMAC would hash such a key first, which is not done
 *                here.
 *     labellen   at most 32; seedlen at most 128 (seeds may be NULL when 0).
 *     outlen     1 .. 256 (the largest key block is 2 48 + 2 32 + 2 16 = 192).
 *     n          at most 2^31.
 *   Every argument error is TG_EINVAL before any HIP call; n == 0 is TG_OK
 *   with nothing launched.  Nothing but out[0, n outlen) is written.  It serves
 *   "key expansion" and "master secret" (seed from the two randoms) and
 *   "extended master secret", "client finished" / "server finished" (seed = a
 *   handshake hash).  The order of the randoms is the caller's business: the
 *   reference uses server_random || client_random for "key expansion" and
 *   client_random || server_random for "master secret" (mathtls.py:900-904).
 *   Kernels on `stream` and library scratch only (two padded message templates
 *   per session, holding label and seed, never the secret).
 *
 * tg_sessions_install_tls12 / tg_cbc_sessions_install_tls12: the TLS 1.2
 *   counterpart of tg_sessions_rekey with TG_REKEY_INSTALL.  For list position
 *   j and slot s = slot[j], the key block
 *     P_hash(master_secrets[j], "key expansion" || server_random[j] ||
 *            client_random[j])
 *   is cut as calcPendingStates cuts it -- client MAC, server MAC, client key,
 *   server key, client IV, server IV -- and the slices of `side` rebuild entry
 *   s of the live handle; the raw keys exist in registers only.
 *     AEAD handle (tg_key, every type tg_sessions_rekey covers, the single-key
 *       AES-GCM handle included): MAC length 0, key length the handle's, IV
 *       length fixed_iv_len: 4 for AES-GCM, AES-CCM, AES-CCM_8 and draft-00
 *       ChaCha20, 12 for RFC 7905 ChaCha20-Poly1305 (_getCipherSettings
 *       :1022-1079).  The IV goes to row s of iv_table (nsessions rows of
 *       fixed_iv_len bytes, the table tg_session_records reads).
 *     CBC handle (tg_cbc_key): the MAC key length is the handle's MAC's digest
 *       length (20 / 32 / 48, _getMacSettings :1081-1102), the key length the
 *       handle's; row s is rebuilt whole, as tg_cbc_key_replace_device does.
 *       The two 16-byte IV blocks that follow in the key block are not
 *       derived: unused at TLS >= 1.1.  fixed_iv_len and iv_table are ignored.
 *   seq_next[s] = 0 when seq_next is given.  hashlen is the suite's PRF hash
 *   (48 for the reference's sha384PrfSuites, else 32).  Only the pairs a
 *   TLS 1.2 suite can produce are built: hashlen 48 goes with an AES-256-GCM
 *   handle or an AES-256-CBC + HMAC-SHA384 handle alone, and an HMAC-SHA384
 *   handle takes no other hashlen; any other pair is TG_EINVAL.  Everything else is
 *   tg_sessions_rekey's contract: a slot >= nkeys is skipped (no table, IV or
 *   counter of it read or written), the slots of one call must be DISTINCT,
 *   ORDERING follows `stream` only (no host synchronisation, no key material
 *   on the host), every byte of a rebuilt entry is overwritten.  Argument
 *   errors (NULL key / struct / master_secrets / client_random /
 *   server_random, AEAD: NULL iv_table or fixed_iv_len other than 4 / 12, bad
 *   hashlen or side, nsessions != nkeys, n > nkeys, n > 2^31, a hashlen no
 *   suite pairs with the handle) are TG_EINVAL before any HIP call; n == 0 is
 *   TG_OK with nothing launched. */
int tg_tls12_prf(int hashlen, const uint8_t* secrets, size_t secretlen, uint64_t n,
                 const uint8_t* label, size_t labellen, const uint8_t* seeds, size_t seedlen,
                 size_t outlen, uint8_t* out, void* stream);
int tg_tls10_prf(const uint8_t* secrets, size_t secretlen, uint64_t n, const uint8_t* label,
                 size_t labellen, const uint8_t* seeds, size_t seedlen, size_t outlen,
                 uint8_t* out, void* stream);

#define TG_TLS12_CLIENT_WRITE 0 /* the client's write keys (a server's read side) */
#define TG_TLS12_SERVER_WRITE 1
typedef struct tg_tls12_install {
    uint64_t n;
    uint32_t hashlen;           /* the suite's PRF hash: 32 or 48 (_tls11: ignored) */
    uint32_t side;              /* which half of the key block */
    uint64_t nsessions;         /* must equal the handle's nkeys */
    const uint32_t* slot;       /* n entries, DEVICE; NULL = 0..n-1 */
    const uint8_t* master_secrets; /* n x 48 */
    const uint8_t* client_random;  /* n x 32 */
    const uint8_t* server_random;  /* n x 32 */
    uint32_t fixed_iv_len;      /* AEAD: 4 or 12; CBC: ignored */
    uint32_t reserved;          /* ignored */
    uint8_t* iv_table;          /* AEAD: nsessions x fixed_iv_len, required; CBC: ignored */
    uint64_t* seq_next;         /* optional: counters of the slots set to 0 */
} tg_tls12_install;
int tg_sessions_install_tls12(tg_key* k, const tg_tls12_install* r, void* stream);

/* The TLS 1.3 key schedule on the device -- what tlsconnection.py runs per
 * connection with hashlib (:3036-3050, :3203-3224, :3326-3360; the client at
 * :1319-1333, :1552-1568, :1659-1701), for many sessions at once: from the
 * (EC)DHE shared secret, an optional PSK and the transcript hashes to the
 * traffic secrets that tg_sessions_rekey (TG_REKEY_INSTALL) installs, with the
 * Finished values and the PSK binders on the way.  One session per lane; every
 * secret between a call's inputs and its outputs exists in registers only.
 *
 * Common to the five calls.  hashlen is 32 (SHA-256) or 48 (SHA-384) and is
 * the size of every secret, salt and transcript-hash row.  All pointers are
 * DEVICE pointers except `label`, which is HOST memory; rows are packed (row i
 * at rowlen * i) and may have any alignment.  n is at most 2^31; n == 0 is
 * TG_OK with nothing launched.  Every argument error (the ones named below, a
 * bad hashlen, n above 2^31, a NULL array that is not optional) is TG_EINVAL
 * with a tg_last_error() reason before any HIP call, length errors first and
 * NULL device arrays after the n == 0 shortcut, as tg_tls12_prf.  Kernels on
 * `stream` only, no host synchronisation, no scratch; nothing is written but
 * [0, n * rowlen) of the named outputs.
 *
 * tg_hkdf_extract: out[i] = HKDF-Extract(salts[i], ikm[i]) =
 *   HMAC-Hash(salt, ikm) (secureHMAC, cryptomath.py:128-132).  salts: n x
 *   hashlen, NULL = hashlen zero bytes for every row.  ikm: n x ikmlen with
 *   ikmlen 1 .. 1024 (every group's shared secret up to ffdhe8192, any
 *   external PSK); NULL = hashlen zero bytes for every row, and ikmlen must
 *   then be 0 or hashlen.  out: n x hashlen.  The IKM is hashed in as many
 *   blocks as ikmlen needs.
 * tg_hkdf_expand_label_rows: tg_hkdf_expand_label with one context per row:
 *   out[i] = HKDF-Expand-Label(secrets[i], label, contexts[i], outlen)
 *   (cryptomath.py:155-173).  label comes without the "tls13 " prefix,
 *   labellen at most 32; contexts: n x ctxlen, ctxlen 0 .. 64; outlen 1 ..
 *   hashlen, out: n x outlen.  contexts == NULL with ctxlen == hashlen means
 *   Hash("") for every row (derive_secret's handshake_hashes None, :175-195);
 *   contexts may otherwise be NULL only when ctxlen is 0.  Derive-Secret is
 *   the case ctxlen == outlen == hashlen with a transcript hash per row.
 * tg_tls13_finished: out[i] = HMAC(HKDF-Expand-Label(secrets[i], "finished",
 *   "", hashlen), hashes[i]) -- the verify_data of Finished (:3210-3216) and,
 *   over a binder key, the PSK binder (handshakehelpers.py:44-61).  secrets,
 *   hashes and out: n x hashlen.  The finished key is never stored.
 * tg_tls13_handshake_secrets (tlsconnection.py:3036-3050), fused:
 *     early   = Extract(0, psk[i])               psk NULL: hashlen zero bytes
 *     derived = Derive-Secret(early, "derived", Hash(""))
 *     hs      = Extract(derived, shared[i])      shared: n x sharedlen, 1 .. 1024
 *   handshake_secret[i] = hs, client_traffic[i] = Derive-Secret(hs,
 *   "c hs traffic", hello_hash[i]), server_traffic[i] = Derive-Secret(hs,
 *   "s hs traffic", hello_hash[i]).  psk: n x hashlen (a PSK of the suite's
 *   hash, as the reference's) or NULL; hello_hash: n x hashlen, the transcript
 *   through ServerHello.  Each of the three outputs (n x hashlen) may be NULL:
 *   not written; all three NULL is an error.
 * tg_tls13_application_secrets (:3218-3224, :3326), fused:
 *     derived = Derive-Secret(handshake_secret[i], "derived", Hash(""))
 *     master  = Extract(derived, hashlen zero bytes)
 *   master_secret[i] = master and, all over finished_hash[i] (the transcript
 *   through the server's Finished), client_traffic[i] = Derive-Secret(master,
 *   "c ap traffic"), server_traffic[i] = ... "s ap traffic",
 *   exporter_master[i] = ... "exp master".  Each of the four outputs may be
 *   NULL: not written; all four NULL is an error.  master_secret may EQUAL
 *   handshake_secret: a lane has read its whole input row before its first
 *   store, so the handshake secrets are overwritten in place.  Any other
 *   overlap of an output's [0, n * hashlen) with an input's or with another
 *   output's is TG_EINVAL.  ("res master" needs the client's Finished in the
 *   transcript: tg_hkdf_expand_label_rows on master_secret, later.)
 * Expand-Label outputs longer than one digest (the exporter's last step) are
 * out of scope. */
int tg_hkdf_extract(int hashlen, const uint8_t* salts, const uint8_t* ikm, size_t ikmlen,
                    uint64_t n, uint8_t* out, void* stream);
int tg_hkdf_expand_label_rows(int hashlen, const uint8_t* secrets, uint64_t n, const uint8_t* label,
                              size_t labellen, const uint8_t* contexts, size_t ctxlen, size_t outlen,
                              uint8_t* out, void* stream);
int tg_tls13_finished(int hashlen, const uint8_t* secrets, const uint8_t* hashes, uint64_t n,
                      uint8_t* out, void* stream);
int tg_tls13_handshake_secrets(int hashlen, const uint8_t* psk, const uint8_t* shared, size_t sharedlen,
                               const uint8_t* hello_hash, uint64_t n, uint8_t* handshake_secret,
                               uint8_t* client_traffic, uint8_t* server_traffic, void* stream);
int tg_tls13_application_secrets(int hashlen, const uint8_t* handshake_secret, const uint8_t* finished_hash,
                                 uint64_t n, uint8_t* master_secret, uint8_t* client_traffic,
                                 uint8_t* server_traffic, uint8_t* exporter_master, void* stream);

/* TLS 1.1 / 1.2 AES-CBC + HMAC records -- the block-cipher suites of
 * RecordLayer._getCipherSettings / _getMacSettings (recordlayer.py:1056-1063,
 * :1087-1095): AES-128 / AES-256 in CBC mode with HMAC-SHA1 / -SHA256 /
 * -SHA384, MAC-then-encrypt (_macThenEncrypt :476-498, _decryptThenMAC
 * :680-719 with ct_check_cbc_mac_and_pad, constanttime.py:102-204) and
 * encrypt-then-MAC, RFC 7366 (_encryptThenMAC :500-520, _macThenDecrypt
 * :721-778).  One connection direction per call: one cipher key, one MAC key,
 * record i has sequence number seq0 + i.  The MAC input is calculateMAC's
 * (:463-474): be64(seq) || type || version(2) || be16(len) || bytes.
 *
 * The key is a handle type of its own (the AEAD handles and their algorithm
 * switches are untouched).  It holds the round keys, the round keys of the
 * equivalent inverse cipher and the two HMAC midstates, built at creation and
 * scrubbed at destroy.  mackeylen is 1 .. the hash's block size (64, SHA-384:
 * 128).  tg_cbc_key_destroy waits for the device first.
 *
 * All arrays of tg_cbc_records are DEVICE pointers; calls are ordered on
 * `stream`.  Every argument error (NULL key or struct, a version other than
 * TG_TLS11 / TG_TLS12, etm > 1, seal without iv, bad key lengths, unknown
 * mac) is TG_EINVAL before any HIP call; n == 0 is TG_OK with nothing
 * launched.
 *   seal: fragment data + data_off[i], data_len[i] bytes (read only; at most
 *         2^14, so that the body fits the header's 16-bit length), content
 *         type ctype[i], explicit IV iv + 16 i (for TLS >= 1.1 the reference
 *         sends a random block first; its ciphertext is this IV).  Writes
 *         header || iv || CBC(data || MAC || padding)        (etm == 0)
 *         header || iv || CBC(data || padding) || MAC        (etm == 1)
 *         at wire + wire_off[i] with the reference's minimal padding
 *         (addPadding :453-461) and its size to wire_len[i]:
 *         5 + 16 + roundup16(len + D + 1), or 5 + 16 + roundup16(len + 1) + D,
 *         D = 20 / 32 / 48.
 *   open: wire record (header included) at wire + wire_off[i], wire_len[i]
 *         bytes.  Plaintext goes to data + data_off[i] (room for
 *         wire_len[i] - 21 bytes), its length to data_len[i], the header's
 *         type to ctype[i] and to status[i] the code of what recvRecord
 *         raises for the record, in the reference's order of checks:
 *         TG_REC_OVERFLOW (header length over recv_limit + 2048, or plaintext
 *         over recv_limit), TG_REC_DECRYPT_FAILED, TG_REC_BAD_MAC (every
 *         TLSBadRecordMAC: MAC mismatch, bad padding, too short, nothing left
 *         after the IV), TG_REC_OK.  Under etm the MAC is checked before the
 *         block-multiple test.  For any status but TG_REC_OK data_len[i] = 0
 *         and every byte written to the record's data extent is zero again.
 *         wire_len[i] < 5 is not even a header: no byte at wire_off[i] is
 *         read, status[i] = TG_REC_BAD_MAC, ctype[i] = 0, data_len[i] = 0
 *         and nothing is written to the data buffer (data_off[i] may point
 *         anywhere).
 *         MAC-then-encrypt costs the same hash blocks and AES blocks whatever
 *         the decrypted bytes are (it depends on wire_len[i] and the MAC).
 * Nothing outside a record's own data and wire extents is written.  Any
 * alignment is accepted; data_off[i] and wire_off[i] + 5 at 16-byte
 * alignment take the vector path. */
#define TG_TLS11 0x0302
#define TG_MAC_SHA1 1
#define TG_MAC_SHA256 2
#define TG_MAC_SHA384 3
#define TG_REC_DECRYPT_FAILED 9 /* TLSDecryptionFailed: body not a multiple of 16 */

typedef struct tg_cbc_key tg_cbc_key;
int tg_cbc_key_create(const uint8_t* enc_key, size_t keylen, const uint8_t* mac_key,
                      size_t mackeylen, int mac, tg_cbc_key** out);
int tg_cbc_key_destroy(tg_cbc_key* k);

typedef struct tg_cbc_records {
    uint64_t n;
    uint32_t version;           /* TG_TLS11 or TG_TLS12 */
    uint32_t etm;               /* 0 = MAC-then-encrypt, 1 = encrypt-then-MAC */
    uint32_t recv_limit;        /* open: recv_record_limit (0 = 2^14) */
    uint32_t reserved;          /* the alignment hole in front of seq0, named; ignored */
    uint64_t seq0;
    uint8_t* data;
    const uint64_t* data_off;
    uint32_t* data_len;
    uint8_t* ctype;
    const uint8_t* iv;          /* seal: n x 16 bytes */
    uint8_t* wire;
    const uint64_t* wire_off;
    uint32_t* wire_len;
    uint8_t* status;            /* open */
} tg_cbc_records;

int tg_cbc_seal_records(tg_cbc_key* k, const tg_cbc_records* r, void* stream);
int tg_cbc_open_records(tg_cbc_key* k, const tg_cbc_records* r, void* stream);

/* AES-CBC + HMAC records of MANY sessions in one batch: the pending records of
 * many RecordLayers of one CBC suite (one direction each) through one call --
 * tg_session_records carried over to tg_cbc_records.  Both chains of a CBC +
 * HMAC record are serial inside the record, so a batch fills the machine only
 * with tens of thousands of records; a server has them spread over many
 * connections, a few each.
 *
 * KEY TABLES.  tg_cbc_key_create_table builds a handle of nkeys rows (cipher
 * key j at enc_keys + j keylen, MAC key j at mac_keys + j mackeylen, HOST
 * memory); keylen, mackeylen and mac hold for every row -- one table, one
 * suite.  The argument errors are tg_cbc_key_create's, and nkeys == 0.
 * tg_cbc_key_create is the table of one row; tg_cbc_key_info reports keylen,
 * mac and nkeys (any out pointer may be NULL).  A table handle passed to
 * tg_cbc_seal_records / tg_cbc_open_records uses row 0.  tg_cbc_key_destroy
 * frees either kind: it waits for the device and scrubs every row.
 *
 * tg_cbc_key_replace: row j of the HOST arrays (n x keylen, n x mackeylen;
 *   mackeylen may differ from creation's, within the MAC's limit) becomes
 *   entry slot[j] (slot in HOST memory, NULL = 0..n-1) of the LIVE handle.
 *   The rows are built on the host, as creation builds them, and copied into
 *   the table ordered on `stream`: batches enqueued on `stream` before the
 *   call use the old rows, batches after it the new ones; work on other
 *   streams must be ordered against it by the caller.  A slot >= nkeys is
 *   skipped; the slots of one call must be DISTINCT.  The call blocks the
 *   host until its copies have left the staging memory (it waits for the
 *   stream's earlier work with them, not for the device) and scrubs the
 *   staging before it returns.  n == 0 is TG_OK; NULL key or arrays, n >
 *   nkeys and a bad mackeylen are TG_EINVAL before any HIP call.  One replace
 *   at a time per handle.
 *
 * tg_cbc_key_create_device / tg_cbc_key_replace_device: the same two calls
 *   with every array in DEVICE memory, slot included (NULL = rows 0..n-1).  A
 *   kernel builds the rows -- the forward schedule, the equivalent inverse
 *   cipher's schedule, the two HMAC midstates -- byte for byte as the host
 *   builds them.  tg_cbc_key_create_device synchronises `stream` before it
 *   returns, as tg_key_create_device does; its argument errors are
 *   tg_cbc_key_create_table's.  tg_cbc_key_replace_device has
 *   tg_key_replace_device's contract: kernels on `stream` and nothing else, no
 *   host synchronisation and no staging; a slot >= nkeys is skipped with
 *   nothing read or written for it; the slots of one call must be DISTINCT;
 *   every byte of a rebuilt row is overwritten; n == 0 is TG_OK; NULL key or
 *   arrays, n > nkeys and a bad mackeylen are TG_EINVAL before any HIP call.
 *   Rows derived from TLS 1.2 master secrets without the raw keys ever being
 *   stored: tg_cbc_sessions_install_tls12, and from TLS 1.1 master secrets
 *   tg_cbc_sessions_install_tls11 (see tg_tls12_install).
 *
 * tg_cbc_seal_session_records / tg_cbc_open_session_records.  All arrays are
 * DEVICE pointers; record i belongs to session s = session[i] and uses table
 * row s.
 *   Per RECORD everything is tg_cbc_records': the wire layout of both
 *   constructions, the minimal padding, the order of open's checks and the
 *   status codes, the wire_len[i] < 5 rule, the zeroed data extent for every
 *   status but TG_REC_OK, "nothing outside a record's own extents is
 *   written", any alignment, and MAC-then-encrypt open costing the same
 *   whatever the decrypted bytes are.  version and etm are one per batch.
 *   Per SESSION everything is tg_session_records': exactly one of seq
 *   (explicit: record i has number seq[i]) and seq_next (counter mode:
 *   nsessions counters; record i gets seq_next[s] as it was before the call
 *   plus the number of earlier records of s in the batch, and seq_next[s]
 *   advances by the session's record count; sessions without records are
 *   untouched; on open every in-range record consumes a number whatever its
 *   status); seq_out is optional and receives the number of every in-range
 *   record; nsessions must equal the handle's nkeys; n <= 2^32 - 2; two calls
 *   that share seq_next must be ordered on one stream.
 *   A record with session[i] >= nsessions is skipped, and that test comes
 *   before every other: nothing of the table, of its iv row or of its data /
 *   wire is read (its offsets may point anywhere) and no number is consumed;
 *   seal writes nothing to wire and sets wire_len[i] = 0; open sets
 *   status[i] = TG_REC_BAD_SESSION, data_len[i] = 0, ctype[i] = 0 and writes
 *   nothing to data.
 * Every argument error (those of tg_cbc_records; both or neither of seq /
 * seq_next; n too large; NULL session; nsessions != nkeys) is TG_EINVAL before
 * any HIP call; n == 0 is TG_OK with nothing launched. */
int tg_cbc_key_create_table(const uint8_t* enc_keys, size_t keylen, const uint8_t* mac_keys,
                            size_t mackeylen, int mac, size_t nkeys, tg_cbc_key** out);
int tg_cbc_key_info(const tg_cbc_key* k, size_t* keylen, int* mac, size_t* nkeys);
int tg_cbc_key_replace(tg_cbc_key* k, const uint32_t* slot, const uint8_t* enc_keys,
                       const uint8_t* mac_keys, size_t mackeylen, uint64_t n, void* stream);
int tg_cbc_key_create_device(const uint8_t* enc_keys, size_t keylen, const uint8_t* mac_keys,
                             size_t mackeylen, int mac, size_t nkeys, tg_cbc_key** out, void* stream);
int tg_cbc_key_replace_device(tg_cbc_key* k, const uint32_t* slot, const uint8_t* enc_keys,
                              const uint8_t* mac_keys, size_t mackeylen, uint64_t n, void* stream);
int tg_cbc_sessions_install_tls12(tg_cbc_key* k, const tg_tls12_install* r, void* stream);
int tg_cbc_sessions_install_tls11(tg_cbc_key* k, const tg_tls12_install* r, void* stream);

typedef struct tg_cbc_session_records {
    uint64_t n;
    uint32_t version;           /* TG_TLS11 or TG_TLS12, one per batch */
    uint32_t etm;               /* one per batch */
    uint32_t recv_limit;        /* open: recv_record_limit (0 = 2^14) */
    uint32_t reserved;          /* ignored */
    uint64_t nsessions;         /* must equal the handle's nkeys */
    const uint32_t* session;
    const uint64_t* seq;        /* exactly one of seq / seq_next */
    uint64_t* seq_next;
    uint64_t* seq_out;          /* optional */
    uint8_t* data;
    const uint64_t* data_off;
    uint32_t* data_len;
    uint8_t* ctype;
    const uint8_t* iv;          /* seal: n x 16 bytes */
    uint8_t* wire;
    const uint64_t* wire_off;
    uint32_t* wire_len;
    uint8_t* status;            /* open */
} tg_cbc_session_records;

int tg_cbc_seal_session_records(tg_cbc_key* k, const tg_cbc_session_records* r, void* stream);
int tg_cbc_open_session_records(tg_cbc_key* k, const tg_cbc_session_records* r, void* stream);

/* Host ingest pipeline (tlsgpu/ingest.py) -- the
 * batched counterpart of RecordSocket (recordlayer.py:35-237).
 * tg_scan_records (HOST memory, no GPU): walk the 5-byte record headers
 *   (RecordHeader3, RecordSocket._recvHeader :169-205) of the wire bytes
 *   buf[0, len): record k starts at off[k] and spans rlen[k] = 5 + body bytes.
 *   Stops at the first incomplete record or after max_n records; *consumed =
 *   the bytes of the complete records.  Returns the record count, or
 *   TG_EOVERFLOW if a header declares body > max_body (TLSRecordOverflow,
 *   RecordSocket.recv :225-229: recv_record_limit + 2048, TLS 1.3 + 256) and
 *   TG_EHEADER for a first byte that is no TLS content type (20..24; the
 *   reference would try SSLv2 framing there).  Records before the bad header
 *   are reported through *consumed and off/rlen (the return value is then
 *   negative, so count them by *consumed).
 * tg_gather (DEVICE memory): for i < n copy len[i] bytes from
 *   src + src_off[i] to dst + dst_off[i] (pack aligned wire records into
 *   one contiguous stream and back).  off/len arrays in device memory. */
#define TG_EOVERFLOW (-75)
#define TG_EHEADER (-71)
int64_t tg_scan_records(const uint8_t* buf, size_t len, uint32_t max_body, uint64_t* off,
                        uint32_t* rlen, size_t max_n, size_t* consumed);
int tg_gather(const uint8_t* src, const uint64_t* src_off, const uint32_t* len, uint8_t* dst,
              const uint64_t* dst_off, uint64_t n, void* stream);
/* tg_host_copy / tg_host_copy_rows (HOST memory, no GPU): the ingest
 *   pipeline's copies between callers' buffers and pinned staging, split over
 *   up to nthreads threads (the caller plus a shared pool of workers;
 *   nthreads <= 0 = min(8, hardware threads)).  rows: row r of row_bytes
 *   bytes goes from src + r * src_stride to dst + r * dst_stride.  Regions
 *   must not overlap.  Returns TG_OK or TG_EINVAL (NULL with a non-zero
 *   size). */
int tg_host_copy(void* dst, const void* src, size_t bytes, int nthreads);
int tg_host_copy_rows(void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t row_bytes,
                      size_t rows, int nthreads);
/* Self-test entry points (TEST-ONLY, not on the record path): run the
 * engine's device Poly1305 / GHASH arithmetic on raw messages, HOST buffers,
 * synchronous, so the reference's known answers reach the exact device code
 * of the AEAD kernels (the reference's Poly1305 / GHASH have no entry point of
 * their own: poly1305.py:32-48 Poly1305.create_tag, aesgcm.py:60-79
 * AESGCM._auth with a zero tag mask).
 * tg_selftest_poly1305: tags[i] = Poly1305(keys[i] (32 B), msgs + off[i],
 *   len[i] bytes) with RFC padding; mode 0 = the lane Horner of the batch
 *   kernel, 1 / 2 / 3 = the wave-striped Horner of the wave-per-record
 *   kernel with 1 / 4 / 16 waves per message, 4 = the octet striping of the
 *   octet kernel (eight lanes per message, chacha_variant 6).
 * tg_selftest_ghash: out[i] = GHASH_H(aad_i, ct_i) (h: n x 16 B, GCM byte
 *   order); mode 0 = 8-bit tables, 1 = 8-bit tables 8 rows in flight,
 *   2 = conflict-free rotated tables, 3 = table-free carry-less multiply,
 *   4 = octet stride-H^8 + lift (aes_gcm_bs8.hip), 5 = wave stride-H^64 +
 *   lift (gcm_wave_kernel), 6 = octet stride-H^8 through a wave's 4-bit
 *   tables (the key-table octet kernel). */
int tg_selftest_poly1305(int mode, const uint8_t* keys, const uint8_t* msgs, const uint64_t* off,
                         const uint32_t* len, uint64_t n, uint8_t* tags);
int tg_selftest_ghash(int mode, const uint8_t* h, const uint8_t* aad, const uint64_t* aad_off,
                      const uint32_t* aad_len, const uint8_t* ct, const uint64_t* ct_off,
                      const uint32_t* ct_len, uint64_t n, uint8_t* out);

/* Diagnostics: the per-launch scratch the library holds (the buffers of
 * its scratch cache, all devices) -- bounded by the launches in flight, not
 * by the streams a caller has used.  Test and monitoring use.
 * A batch call borrows a scratch buffer and gives it back behind its work
 * on the caller's stream; the next call on the same stream handle may take
 * it again at once, and that call's stream then waits for the buffer's
 * last work, so a stream destroyed with work pending and a new stream that
 * receives its handle stay correct.
 * tg_scratch_trim: frees cached scratch buffers whose work has completed
 *   until at most keep_bytes remain, and every idle helper stream (the
 *   second stream a key-table batch runs its short records on).  The cache
 *   also trims itself before it grows past 8 GiB.
 * tg_helper_info: helper streams the library holds, and how many a batch
 *   is using right now (one per caller stream in flight, at most). */
int tg_scratch_info(uint64_t* bytes, uint64_t* buffers);
int tg_scratch_trim(uint64_t keep_bytes);
int tg_helper_info(uint64_t* streams, uint64_t* busy);

/* Device memory helpers so a ctypes host needs no other GPU runtime. */
int tg_malloc(void** p, size_t bytes);
int tg_free(void* p);
int tg_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int tg_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int tg_stream_sync(void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
