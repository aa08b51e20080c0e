/*
 * fpnn_aes.h -- C-ABI of the MI355X AES-CFB packet-encryption path.
 *
 * Replaces, for batches of independent packets/streams, the CPU path
 *   core/Encryptor.cpp:10-70  (PackageEncryptor / StreamEncryptor)
 *     -> base/rijndael.c:1171-1201 (rijndael_cfb_encrypt)
 *        -> base/rijndael.c:852-959 (rijndael_encrypt)
 * of the reference (highras/fpnn v1.3.1).  Plain pointers and sizes only;
 * no exceptions and no C++/torch types cross this boundary.  Every call
 * returns an int status (the reference functions are void; see
 * FPNN_AES_ERR_* below for what is now reported instead of being undefined).
 *
 * Device pointers ("dev") are HIP device addresses on the engine's GPU; host
 * pointers ("host") are ordinary process memory.  All device work is queued on
 * the engine's HIP stream; calls return after queuing unless they say otherwise.
 * Results are bit-identical to the reference for every key length (16/24/32),
 * payload length (including 0 and non-multiples of 16) and CFB position.
 *
 * Library layout: libfpnn_aes.so (what callers link) carries these entry points, the
 * C++ classes (Encryptor.h, EncryptorBatch.h, StreamReceiverBatch.h, KeyExchange.h) and
 * no HIP dependency of its own; on first use it loads libfpnn_aes_gpu.so from its own
 * directory (FPNN_AES_GPU_LIB overrides the path) -- the HIP kernels and the engine --
 * and forwards every call there.  Loading the HIP runtime late keeps its static TLS
 * (about 30 KiB, rocprofiler-register) out of every thread's stack: FPNN starts threads
 * with 16 KiB stacks (base/msec.c:72-74), which the runtime linked at start-up made
 * pthread_create refuse.  If the GPU library cannot be loaded every call returns
 * FPNN_AES_ERR_NODEV (fpnn_aes_last_error says why).
 */
#ifndef FPNN_AES_H
#define FPNN_AES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------- */
#define FPNN_AES_OK            0
#define FPNN_AES_ERR_KEYLEN   -1  /* key length not 16/24/32 (reference: setup returns false
                                     and the cipher then runs with nrounds = 0, rijndael.c:797) */
#define FPNN_AES_ERR_ARG      -2  /* NULL pointer, bad descriptor, mixed key lengths */
#define FPNN_AES_ERR_RANGE    -3  /* batch too large (more than 2^32-1 16-byte blocks or packets) */
#define FPNN_AES_ERR_HIP      -4  /* HIP runtime error (message: fpnn_aes_last_error) */
#define FPNN_AES_ERR_NODEV    -5  /* no usable gfx950 device / kernels not loadable */
#define FPNN_AES_ERR_DEVICE   -6  /* a queued kernel's own consistency check failed (reported by
                                     the next fpnn_aes_engine_sync or synchronous call) */

const char *fpnn_aes_strerror(int status);
/* Thread-local text of the last HIP error seen by this thread (or ""). */
const char *fpnn_aes_last_error(void);

/* ---- key schedule ------------------------------------------------------------ */
/* Layout identical to rijndael_context (base/rijndael.h:13-16). */
typedef struct {
    int nrounds;
    uint32_t rk[60];
} fpnn_aes_schedule;

/* Host key expansion.  Mirrors rijndael_setup_encrypt (base/rijndael.c:712-799):
 * same big-endian rk[] words, same nrounds; returns FPNN_AES_OK or
 * FPNN_AES_ERR_KEYLEN (and sets nrounds = 0, like the reference). */
int fpnn_aes_setup_encrypt(fpnn_aes_schedule *ctx, const uint8_t *key, size_t keylen);

/* Decryption key schedule.  Mirrors rijndael_setup_decrypt (base/rijndael.c:805-850):
 * the encryption schedule with the round keys reversed and InvMixColumns applied to all
 * but the first and last -- the same rk[] words as the reference. */
int fpnn_aes_setup_decrypt(fpnn_aes_schedule *ctx, const uint8_t *key, size_t keylen);

/* ---- engine: one GPU, one HIP stream ---------------------------------------- */
typedef struct fpnn_aes_engine fpnn_aes_engine;
#define FPNN_AES_OWN_STREAM ((void *)(intptr_t)-1)

int fpnn_aes_device_count(int *count);
/* hip_stream: the hipStream_t to queue on (e.g. torch's current stream); NULL is
 * the device's null stream, as everywhere in HIP; FPNN_AES_OWN_STREAM creates a
 * private non-blocking stream owned by the engine.  The engine is not thread-safe; use one
 * engine per submitting thread (the reference's per-connection token discipline,
 * core/IOBuffer.h:49-62, makes each Encryptor single-threaded in the same way). */
int fpnn_aes_engine_create(int device, void *hip_stream, fpnn_aes_engine **out);
int fpnn_aes_engine_destroy(fpnn_aes_engine *e);
int fpnn_aes_engine_sync(fpnn_aes_engine *e);
void *fpnn_aes_engine_stream(fpnn_aes_engine *e);
/* Pre-size scratch for batches of up to max_segments packets/streams and
 * max_blocks total 16-byte blocks, so later device-batch calls of that size never
 * allocate or memset.  They are then graph-safe: a call captured on the engine's stream
 * (hipStreamBeginCapture) may be replayed with new data, offsets and lengths in the same
 * device arrays, because every piece of cross-call scratch state (the block map's
 * look-back epoch and tickets, the length-order block and K2h's tickets) is reset on the
 * device by the kernels that use it (tests/test_gpu_graph.py).  The *_frames stream calls'
 * per-segment scratch is sized from max_segments as well, and so is the scratch of
 * fpnn_ecdh_accept (fpnn_ecdh.h) for up to max_segments peers per call. */
int fpnn_aes_engine_reserve(fpnn_aes_engine *e, uint64_t max_segments, uint64_t max_blocks);
/* Bytes of device scratch the engine holds now (every growing buffer's capacity; 0 for NULL).
 * It changes only when a call grows a buffer: equal values before and after a call mean the
 * call allocated no scratch, which is what fpnn_aes_engine_reserve promises within its bounds. */
uint64_t fpnn_aes_engine_scratch_bytes(fpnn_aes_engine *e);

/* Placement of the engines behind the C++ classes (Encryptor, EncryptorBatch,
 * StreamReceiverBatch, ECCKeyExchange): one pool per process, engine k created on the
 * device returned here for (k, ndev = fpnn_aes_device_count) -- k % ndev, or the k-th
 * entry (cyclically) of the comma list FPNN_AES_DEVICES, or FPNN_AES_DEVICE alone;
 * -1 when no device is usable.  Pure functions of their arguments and the environment
 * (no HIP call), so the plan can be checked without a GPU. */
int fpnn_aes_thread_engine_device(uint32_t k, int ndev);
/* Engines the pool creates before calling threads start to share one (calls on a shared
 * engine serialise): FPNN_AES_MAX_ENGINES, default 16 per usable device, at least 1. */
int fpnn_aes_max_thread_engines(int ndev);

/* ---- key sets: the per-connection (key, IV) table on the device -------------- */
/* A key set holds `count` expanded keys of ONE key length plus one 16-byte IV each
 * (the connection IV of package mode, core/Encryptor.h:14).  keys: count*keylen
 * bytes, ivs: count*16 bytes (NULL => zero IVs).  keys_on_host != 0 means keys/ivs
 * are host pointers (copied), otherwise device pointers.  Expansion runs on the GPU. */
typedef struct fpnn_aes_keyset fpnn_aes_keyset;

int fpnn_aes_keyset_create(fpnn_aes_engine *e, uint32_t count, size_t keylen, const uint8_t *keys,
                           const uint8_t *ivs, int keys_on_host, fpnn_aes_keyset **out);
/* Same, from host schedules already expanded by fpnn_aes_setup_encrypt /
 * rijndael_setup_encrypt (all with the same nrounds). */
int fpnn_aes_keyset_from_schedules(fpnn_aes_engine *e, uint32_t count, const fpnn_aes_schedule *ctx,
                                   const uint8_t *ivs, fpnn_aes_keyset **out);
/* A key table updated in place -- the collector's persistent per-connection table
 * (fpnn::EncryptorBatch): `capacity` slots of one key length (nrounds 10/12/14), all zero.
 * fpnn_aes_keyset_set writes host schedules (+ IVs, NULL => zero) into slots
 * [first, first + count), growing the table when needed (contents kept); it is queued on
 * the engine stream through pinned staging, so a flush that adds a few connections
 * costs one small copy and no allocation.  The key set's count becomes
 * max(count, first + count). */
int fpnn_aes_keyset_reserve(fpnn_aes_engine *e, uint32_t capacity, int nrounds, fpnn_aes_keyset **out);
int fpnn_aes_keyset_set(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const fpnn_aes_schedule *ctx,
                        const uint8_t *ivs);
uint32_t fpnn_aes_keyset_count(const fpnn_aes_keyset *ks);
int fpnn_aes_keyset_destroy(fpnn_aes_keyset *ks);
int fpnn_aes_keyset_nrounds(const fpnn_aes_keyset *ks);
/* Copy the expanded schedule of slot i back to the host (rijndael_context layout). */
int fpnn_aes_keyset_get_schedule(fpnn_aes_keyset *ks, uint32_t slot, fpnn_aes_schedule *out);

/* ---- accept and retire connections in a LIVE table, on the device ------------- */
/* Slots the table's allocations hold: the reserved (or grown) capacity; for a key set made
 * by _create / _from_schedules, its count until a call below grows it.  0 for NULL. */
uint32_t fpnn_aes_keyset_capacity(const fpnn_aes_keyset *ks);
/* fpnn_aes_keyset_set_keys: `count` RAW keys of the table's key length (keys: DEVICE,
 * count * keylen bytes, any alignment) and their IVs (ivs: DEVICE, count * 16 bytes, or
 * NULL => zero IVs) are expanded on the device (rijndael_setup_encrypt's schedule,
 * base/rijndael.c:712-799) and written, with the slot's first keystream block, into
 *     slot s_i = slots ? slots[i] : first + i        (slots: DEVICE, 4-byte aligned, or NULL)
 * An entry with ok != NULL and ok[i] == 0 (ok: DEVICE, count bytes) writes nothing: the slot
 * keeps what it held.
 * fpnn_aes_keyset_clear: the named slots become bit for bit what a never-set slot of
 * fpnn_aes_keyset_reserve holds (a closed connection's key stops existing).
 *
 * Both work on any key set and are QUEUED on the stream of the engine that made the key
 * set, like a batch call: batches queued before the call see the old slots, batches queued
 * after it the new ones; no key byte passes through host memory.
 *
 * The bound known to the host is first + count when slots is NULL and slot_bound otherwise
 * (slot_bound is not used when slots is NULL).  When it exceeds fpnn_aes_keyset_capacity the
 * table grows exactly as fpnn_aes_keyset_set grows it (contents kept; that waits for the
 * stream once); otherwise the call allocates nothing and waits for nothing.  The key set's
 * count becomes max(count, bound).  slot_bound may be below the capacity; the kernels
 * check against slot_bound: an entry with slots[i] >= slot_bound writes nothing, the other
 * entries of the call are written, and the next fpnn_aes_engine_sync returns
 * FPNN_AES_ERR_DEVICE (once; the engine stays usable).  Naming one slot twice in one call is
 * the caller's error: which entry the slot ends up with is not defined.
 * FPNN_AES_ERR_ARG: ks NULL, keys NULL with count != 0, slots not 4-byte aligned;
 * FPNN_AES_ERR_RANGE: first + count past 2^32 - 1.  count == 0 is FPNN_AES_OK and a no-op. */
int fpnn_aes_keyset_set_keys(fpnn_aes_keyset *ks, uint32_t first, uint32_t count,
        const uint32_t *slots, uint32_t slot_bound,      /* dev or NULL; bound used only with slots */
        const uint8_t *keys, const uint8_t *ivs, const uint8_t *ok);   /* all dev; ivs, ok may be NULL */
int fpnn_aes_keyset_clear(fpnn_aes_keyset *ks, uint32_t first, uint32_t count,
        const uint32_t *slots, uint32_t slot_bound);

/* ---- batch descriptor ---------------------------------------------------------- */
/* A batch is `count` independent segments.  Segment i reads len_i bytes at
 * in + in_off[i] and writes len_i bytes at out + out_off[i]:
 *   in_off  == NULL -> in_off[i]  = i * stride
 *   out_off == NULL -> out_off[i] = in_off[i]
 *   len     == NULL -> len_i      = uniform_len
 *   key_slot== NULL -> slot_i     = 0            (index into the key set)
 * Offsets/lengths/slots are device arrays.  `in` and `out` may be the same
 * buffer with identical offsets (in-place: in == out as pointers); any other overlap
 * -- including in != out pointers whose ranges meet -- is undefined. */
typedef struct {
    const uint8_t *in;          /* dev */
    uint8_t *out;               /* dev */
    uint32_t count;
    uint32_t uniform_len;
    uint64_t stride;
    const uint64_t *in_off;     /* dev, optional */
    const uint64_t *out_off;    /* dev, optional */
    const uint32_t *len;        /* dev, optional */
    const uint32_t *key_slot;   /* dev, optional */
    const fpnn_aes_keyset *keys;
    uint32_t flags;             /* FPNN_AES_F_* */
    uint32_t max_len;           /* optional: an upper bound on every len_i in bytes, 0 = unknown.
                                   Ragged package encrypts of many short frames (max_len <=
                                   2048, count >= 1 chain per GPU lane, i.e. 256 CUs x 1024)
                                   then run one lane per chain in grid-stride order (K2;
                                   with max_len <= 175, FPNN's quests, K2s-DB: each frame
                                   loaded, ciphered and stored whole in one pass, the next
                                   one loading meanwhile; package decrypts with that bound
                                   likewise, D2s);
                                   without the bound, or with fewer chains, the
                                   length-ordered hybrid (K2h), whose work queue also balances
                                   Zipf-like lengths.  (Was `reserved`, 0: same layout.) */
} fpnn_aes_batch;

/* Package encrypt only: write the wire frame of PackageEncryptor::encrypt(std::string*)
 * (core/Encryptor.cpp:34-51): htole32(len) at out + out_off[i], ciphertext at +4. */
#define FPNN_AES_F_WIRE_PREFIX 0x1u

/* ---- package mode (core/Encryptor.cpp:10-51) ------------------------------------- */
/* Every segment starts a fresh CFB chain from its key slot's IV at position 0,
 * exactly as PackageEncryptor re-copies _iv and re-expands the key per call.
 * Decrypt runs one GPU lane per 16-byte block; encrypt one lane per packet chain. */
int fpnn_aes_package_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b);
int fpnn_aes_package_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b);

/* ---- stream mode (core/Encryptor.cpp:53-70) ---------------------------------------- */
/* Segment i continues the CFB stream whose state is (iv_state[16*i .. +16],
 * pos_state[i]) -- StreamEncryptor::_iv and ::_pos -- with key slot slot_i; the
 * state is updated in place (dev arrays).  A given stream must appear at most once
 * per call; successive frames of a stream go in successive calls of these two -- or all
 * in one call of the *_frames pair below. */
int fpnn_aes_stream_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state,
                            uint32_t *pos_state);
int fpnn_aes_stream_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state,
                            uint32_t *pos_state);

/* Many frames of each stream in one call (a connection's send queue holds several frames
 * per IO cycle, core/IOBuffer.cpp:47-74).  Stream j owns segments [first_frame[j],
 * first_frame[j+1]) of b, its frames in order: first_frame[0] == 0, first_frame[nstreams]
 * == b->count, non-decreasing.  Results and the final state equal that many successive
 * StreamEncryptor::encrypt / decrypt calls on (iv_state[16*j .. +16], pos_state[j]); the
 * state arrays have nstreams entries, indexed by stream (not by segment).  A stream with no
 * segments, or only empty ones, keeps its state bit for bit.  Segments are described as in
 * every batch (anywhere, in any memory order, with gaps; in place as above); key_slot[] stays
 * per segment, all frames of a stream must name the same slot and the kernels read any one
 * of them.  FPNN_AES_F_WIRE_PREFIX, a NULL first_frame, NULL or misaligned state with
 * nstreams != 0: FPNN_AES_ERR_ARG.  nstreams == 0 or b->count == 0 queues nothing.  Queue-
 * only like the pair above.  A first_frame that is not monotone or does not span [0, count]
 * never makes a kernel leave the batch (what is read from it is clamped): the call's results
 * are then invalid and the next fpnn_aes_engine_sync returns FPNN_AES_ERR_DEVICE. */
int fpnn_aes_stream_encrypt_frames(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                   uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state);
int fpnn_aes_stream_decrypt_frames(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                   uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state);

/* ---- stream mode by key-table slot: open, cipher, close ------------------------------ */
/* A connection that lives in slot s of a live key table keeps its stream state at entry s
 * of the caller's state arrays, so one index names the key and the state, as key_slot does
 * in fpnn_aes_stream_host.  The arrays are the caller's (DEVICE; iv_state 16-byte aligned,
 * 16 bytes per slot; pos_state 4 bytes per slot) and hold at least the call's bound; a
 * connection has two pairs, send and receive.  The life of a connection on the device:
 *
 *   fpnn_ecdh_accept / fpnn_aes_keyset_set_keys     key and IV into slot s
 *   fpnn_aes_stream_open  x 2 (send pair, recv pair) state of s = (IV of s, 0)
 *   fpnn_aes_stream_*_frames_at / _recv_at           per IO cycle, the active slots only
 *   fpnn_aes_stream_encrypt_at / _decrypt_at         the same with one frame per slot
 *   fpnn_aes_stream_host_at                          the same from host socket buffers
 *   fpnn_aes_keyset_clear + fpnn_aes_stream_close x 2   key and state of s are zero
 *
 * fpnn_aes_stream_open: iv_state[16*s_i .. +16] = the IV slot s_i holds, pos_state[s_i] = 0
 * -- what a StreamEncryptor starts from (core/Encryptor.h:44-61) -- for
 *     s_i = slots ? slots[i] : first + i              (slots: DEVICE, 4-byte aligned, or NULL)
 * skipping entries with ok != NULL and ok[i] == 0 (the ok[] of fpnn_ecdh_accept: a refused
 * peer's state is not touched).  A never-set or cleared slot gives an all-zero state.
 * fpnn_aes_stream_close: the state of every s_i becomes all zero (the last ciphertext block
 * and the position of a closed connection stop existing).
 * Both are queued on the stream of the engine that made the key set, read the table, allocate
 * nothing and wait for nothing; entries of the state arrays that are not named keep every bit.
 * The bound is first + count, or slot_bound with slots; neither call grows the table: a bound
 * above fpnn_aes_keyset_capacity is FPNN_AES_ERR_ARG.  An entry with slots[i] >= slot_bound
 * writes nothing, the other entries are written, and the next fpnn_aes_engine_sync returns
 * FPNN_AES_ERR_DEVICE once (as fpnn_aes_keyset_set_keys).  FPNN_AES_ERR_ARG also: ks NULL; with
 * count != 0, NULL or misaligned iv_state / pos_state / slots.  count == 0: FPNN_AES_OK, no-op. */
int fpnn_aes_stream_open(fpnn_aes_keyset *ks, uint32_t first, uint32_t count,
        const uint32_t *slots, uint32_t slot_bound, const uint8_t *ok,   /* dev or NULL */
        uint8_t *iv_state, uint32_t *pos_state);                         /* dev */
int fpnn_aes_stream_close(fpnn_aes_keyset *ks, uint32_t first, uint32_t count,
        const uint32_t *slots, uint32_t slot_bound,
        uint8_t *iv_state, uint32_t *pos_state);

/* fpnn_aes_stream_encrypt_frames / _decrypt_frames with stream j's state at entry
 * state_slot[j] of the state arrays (which hold slot_bound entries) and the key of all its
 * frames in slot state_slot[j] of b->keys (state_slot: DEVICE, nstreams entries, 4-byte
 * aligned).  b->key_slot must be NULL and state_slot must not be (with nstreams != 0), and
 * slot_bound must not exceed fpnn_aes_keyset_capacity(b->keys): FPNN_AES_ERR_ARG otherwise.
 * Everything else is as for the *_frames pair.  Entries of the state arrays the call does
 * not name keep every bit; naming one slot twice in one call is the caller's error.  A
 * stream with state_slot[j] >= slot_bound has its state neither read nor written; encrypt
 * writes nothing for it, decrypt leaves the output bytes of its own segments unspecified
 * and touches no other byte; the other streams are exact, and the next
 * fpnn_aes_engine_sync returns FPNN_AES_ERR_DEVICE once. */
int fpnn_aes_stream_encrypt_frames_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                      uint32_t nstreams, const uint32_t *state_slot, uint32_t slot_bound,
                                      uint8_t *iv_state, uint32_t *pos_state);
int fpnn_aes_stream_decrypt_frames_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                      uint32_t nstreams, const uint32_t *state_slot, uint32_t slot_bound,
                                      uint8_t *iv_state, uint32_t *pos_state);

/* The common IO cycle by slot: ONE frame per stream.  Segment i of b is the one pending frame of
 * the connection in slot state_slot[i] (state_slot: DEVICE, b->count entries, 4-byte aligned):
 * its key is slot state_slot[i] of b->keys, its state entry state_slot[i] of the state arrays
 * (DEVICE, slot_bound entries, iv_state 16-byte aligned), updated in place.  Results and final
 * state equal fpnn_aes_stream_encrypt / _decrypt on state gathered from those entries with
 * key_slot = state_slot -- without the gather and the scatter.
 * Encrypt takes fpnn_aes_stream_encrypt's dispatch unchanged -- one chain per lane (K2), one
 * per lane quad (K2c), or, for ragged batches with more chains than the chip has quads, the
 * length-ordered quad and lane queues (K2h) that balance heavy-tailed frame lengths, which the
 * *_frames_at walk in stream order does not; b->max_len applies as it does there -- and runs
 * the kernel in its slot-addressed form.  Decrypt is fpnn_aes_stream_decrypt_frames_at with one
 * frame per stream (what fpnn_aes_stream_recv_at runs before its scan); the dense whole-stream
 * decrypt kernels of fpnn_aes_stream_decrypt are not reachable by slot.
 * FPNN_AES_ERR_ARG: b->key_slot not NULL; with b->count != 0, state_slot NULL or not 4-byte
 * aligned, iv_state / pos_state NULL or misaligned; slot_bound above
 * fpnn_aes_keyset_capacity(b->keys); FPNN_AES_F_WIRE_PREFIX set.  b->count == 0 queues nothing.
 * Queued on the engine's stream; after fpnn_aes_engine_reserve(max_segments, max_blocks) a call
 * within those bounds allocates nothing (it may be captured in a graph).  Entries of the state
 * arrays the call does not name keep every bit; naming one slot twice in one call is the
 * caller's error.  A segment with state_slot[i] >= slot_bound has its state neither read nor
 * written; encrypt writes no byte of it, decrypt leaves the output bytes of that segment
 * unspecified and touches no other byte; the other segments are exact, and the next
 * fpnn_aes_engine_sync returns FPNN_AES_ERR_DEVICE once. */
int fpnn_aes_stream_encrypt_at(fpnn_aes_engine *e, const fpnn_aes_batch *b,
        const uint32_t *state_slot, uint32_t slot_bound,   /* dev, b->count entries */
        uint8_t *iv_state, uint32_t *pos_state);           /* dev, slot_bound entries */
int fpnn_aes_stream_decrypt_at(fpnn_aes_engine *e, const fpnn_aes_batch *b,
        const uint32_t *state_slot, uint32_t slot_bound,
        uint8_t *iv_state, uint32_t *pos_state);

/* ---- UDP v2 datagrams with data ("enhanced") encryption ------------------------------ */
/* A UDPEncryptor with reinforced data encryption holds two ciphers (core/UDP.v2/
 * UDPCommon.v2.h:100-129, UDPCommon.v2.cpp:146-215): a StreamEncryptor under the data key
 * ciphers each non-discardable data section as the assembler places it into the datagram --
 * ONE CFB chain through the connection's whole life (UDPAssembler.v2.cpp:575-578, 619-622,
 * 698-701) -- and a PackageEncryptor under the package key then ciphers the whole datagram
 * with a fresh chain from the connection IV (UDPIOBuffer.v2.cpp:351); the receiver undoes
 * them in the opposite order (UDPParser.v2.cpp:91, then :702, :773, :827 per section).
 *
 * b describes the DATAGRAMS, as any batch (anywhere, gaps allowed, in place when in == out;
 * bytes of out outside the datagrams are not touched); b->keys is the package table and
 * b->key_slot must be NULL: connection j's slot conn_slot[j] names its key and IV in b->keys,
 * its data key in data_keys, and its entry of the state arrays, which hold the data
 * StreamEncryptor's (_iv, _pos) (fpnn_aes_stream_open on data_keys starts them).  The result
 * is bit for bit the reference's: per connection the datagrams in order, per datagram the
 * sections in order; encrypt = dataEncrypt(section) continuing the slot's state, then
 * packageEncrypt(datagram); decrypt = packageDecrypt(datagram), then dataDecrypt(section).
 * The state is updated in place; slots not named, connections without datagrams and
 * connections whose sections are all empty keep every bit of it.  Datagrams without
 * sections, zero-length datagrams and zero-length sections are legal.  The two tables may
 * have different key lengths, 16 or 32 bytes each (FPNN_AES_ERR_KEYLEN for a 24-byte table).
 *
 * first_dgram and first_section have first_frame's contract (non-decreasing, from 0, ending
 * at b->count / nsections); inside a datagram the sections ascend, do not overlap and lie
 * inside it.  Input that breaks this never makes a kernel leave the datagram's own bytes
 * (what is read is clamped): that connection's results are invalid and the next
 * fpnn_aes_engine_sync returns FPNN_AES_ERR_DEVICE once.  conn_slot[j] >= slot_bound is
 * treated as by fpnn_aes_stream_*_frames_at: the connection's state is not touched, encrypt
 * writes nothing for it, decrypt leaves its own output bytes unspecified, all other
 * connections are exact, FPNN_AES_ERR_DEVICE once.
 *
 * FPNN_AES_ERR_ARG: b->key_slot not NULL, b->flags not 0, u NULL; data_keys NULL with
 * nsections != 0, or made on another engine; with nconn != 0, NULL or misaligned
 * first_dgram, conn_slot, iv_state (16 bytes) or pos_state; with nsections != 0, NULL or
 * misaligned first_section, sec_off or sec_len; slot_bound above the capacity of either
 * table.  nconn == 0 or b->count == 0 queues nothing.  Both calls are queued on the engine's
 * stream with no host wait; after fpnn_aes_engine_reserve(max_segments, max_blocks) with
 * max_segments >= max(b->count, nsections, nconn) they allocate nothing.
 *
 * Encrypt is one kernel (K2u: one lane quad per connection, both key schedules and the data
 * layer's state in registers; no intermediate copy of the batch).  Decrypt queues the
 * package decrypt of the datagrams and the slot-addressed *_frames decrypt of the sections,
 * in place in out, behind one small kernel that derives their descriptors on the device. */
typedef struct {
    const fpnn_aes_keyset *data_keys;  /* data keys (+ data IVs), one key length (16 or 32), same engine */
    uint32_t nconn;                    /* connections in this call */
    const uint32_t *first_dgram;       /* dev, nconn+1: connection j owns datagrams [first_dgram[j], first_dgram[j+1]) of b, in send order */
    const uint32_t *conn_slot;         /* dev, nconn: slot of b->keys, of data_keys AND of the state arrays */
    uint32_t slot_bound;
    uint32_t nsections;
    const uint32_t *first_section;     /* dev, b->count+1: datagram i owns sections [first_section[i], first_section[i+1]) */
    const uint32_t *sec_off;           /* dev, nsections: byte offset inside its datagram */
    const uint32_t *sec_len;           /* dev, nsections */
    uint8_t  *iv_state;                /* dev, 16*slot_bound, 16-byte aligned: the data StreamEncryptor's _iv */
    uint32_t *pos_state;               /* dev, slot_bound: its _pos */
} fpnn_aes_udp_data;

int fpnn_aes_udp_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u);
int fpnn_aes_udp_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u);

/* ---- UDP v2 receive: walk the packages on the device, then decrypt (§8f row 2) -------- */
/* fpnn_aes_udp_decrypt needs the data sections' places, which a receiver learns only from the
 * package-decrypted datagram.  These two calls package-decrypt the datagrams, walk UDP v2's
 * package and component structure as ARQParser does (core/UDP.v2/UDPParser.v2.cpp: parse
 * :59-122, processAssembledPackage :124-159, processPackage :313-346, parseCOMBINED :528-587,
 * the header arithmetic of parseDATA :672-742, parseACKS :840-870, parseUNA :872-892), report
 * it in three small device tables, and data-decrypt the DATA sections of the packages the
 * host's ARQ accepts, continuing each connection's data chain.
 *
 * b and u are fpnn_aes_udp_decrypt's (b->key_slot NULL; conn_slot names the package key, the
 * data key and the state entry), except that the sections are outputs: u->first_section,
 * u->sec_off and u->sec_len must be NULL and u->nsections 0.  u->data_keys may be NULL only
 * with FPNN_AES_UDP_F_WALK_ONLY.  scan has b->count entries, pkgs b->count * max_pkgs,
 * sections b->count * max_sections (device arrays; both products must fit 32 bits); datagram
 * i's rows start at i * max_pkgs and i * max_sections; entries past the used counts are not
 * written.  b->out holds the package-decrypted bytes of every datagram, whatever its status.
 *
 * The walk, per datagram (it reads the datagram's own bytes only, whatever they hold):
 *   len < 8: FPNN_AES_UDP_SHORT, no package.  len > 65535: FPNN_AES_UDP_LONG, no package (no
 *   UDP datagram is; the tables' offsets are 16 bits).  Version byte > 2: FPNN_AES_UDP_VERSION,
 *   no package; otherwise the version is recorded.  Type 0x81 (ARQ_ASSEMBLED): from offset 2,
 *   included packages [be16 length][type flag sign seq4 payload], each one a package row with
 *   the reference's _buffer / _bufferLength (:133-134): off = the length field's second byte,
 *   len = length + 1.  Any other type: one package over the whole datagram (off 0).
 *   Package, by type: COMBINED (0x80) needs len >= 16; its components start at offset 8, each
 *   [type flag be16 bytes] with offset + 4 + bytes <= len, of type DATA, ACKS, UNA, FORCESYNC
 *   or CLOSE.  A whole package may also be a HEARTBEAT.  ECDH (these calls serve encrypted
 *   connections, and the reference refuses ECDH on one, :928-933) and every other type:
 *   FPNN_AES_UDP_TYPE.  ACKS whose bytes are no multiple of 4: FPNN_AES_UDP_ACKS.  A whole-
 *   package UNA needs len == 12.  A UNA component inside COMBINED is accepted as the reference
 *   accepts it, whenever the 4 bytes after its header lie inside the package (:888 reads them
 *   whatever `bytes` says): its section's len is the component's `bytes`, which may be less
 *   than 4 -- the UNA value is then the 4 bytes at off all the same, running into the next
 *   component; a host ARQ reads 4 bytes at off, not len bytes.  CLOSE is recorded as a section and ends its PACKAGE with
 *   status FPNN_AES_UDP_CLOSE, which the ARQ accepts (:336-340, :567-571): the datagram's walk
 *   goes on with the next included package and the datagram's status stays OK.
 *   DATA: flag & 0x0c selects no segment header (0) or packageId (be16) + a 1- (0x04), 2-
 *   (0x08) or 4-byte (0x0c) big-endian index; off / len are the bytes after that header.
 *   Wherever the reference would read a byte outside the package or wrap an unsigned length
 *   the status is FPNN_AES_UDP_SHORT at that point: a component header or a combined UNA's 4
 *   bytes that cross the package's end, a segment header longer than its section (a cancelled
 *   one included: the reference reads only its packageId, but no sender writes less than the
 *   whole header), an included package of length < 7 or one that runs past the datagram, a
 *   1-byte remainder after the last included package.  An included package that is SHORT in
 *   one of these last three ways gets no row (its header is not all there): the datagram's
 *   status carries it.
 *   A rejected package keeps the sections recorded before the point of rejection (the
 *   reference has processed them by then), carries the reason in its status, and ends the
 *   datagram's walk (:150-151, :580-581) with the same status for the datagram.  When a row
 *   has no room for the next entry the status (package and datagram) is FPNN_AES_UDP_FULL;
 *   what fits is recorded.
 *
 * Data decrypt: a section is decrypted when it is DATA without ARQ_Discardable (0x01) and
 * without ARQ_CancelledPackage (0x80) (:695-703, :714, :769-775, :823-829), in place in b->out,
 * continuing the slot's (iv_state, pos_state), which is updated in place.
 *   fpnn_aes_udp_recv without WALK_ONLY takes every package of every datagram in array order:
 *   the single-call form for a caller that has established processing order already.
 *   fpnn_aes_udp_recv_take takes connection j's packages take[first_take[j] .. first_take[j+1])
 *   in that order, each a global package index i * max_pkgs + k of one of the connection's own
 *   datagrams (first_take: device, nconn + 1 entries, first_frame's contract over ntake; take:
 *   device, ntake entries).  It follows a WALK_ONLY call once the host's ARQ has read pkgs[]
 *   (b, u, max_pkgs, max_sections and the tables as in that call), or a PLAIN | WALK_ONLY call
 *   for datagrams that came back from the disordered cache.
 * Connections with nothing to decrypt, slots not named, and everything under WALK_ONLY keep
 * every bit of their state.
 *
 * Why the split is exact: once data encryption is on the reference parses in order
 * (:978): reliable packages are processed strictly by sequence and out-of-order ones are
 * cached as package-plaintext and processed later (:225-250).  A walk that needs no data
 * layer, then "decrypt these packages' sections in this order", is what it does.
 *
 * Limits.  ARQ decisions stay on the host: sequence order, the ARQ checksum
 * (UDPCommon.v2.cpp:6-36), the disordered cache, segment assembly; so does the ECDH-copy filter
 * (:76-89), which the caller applies before the call.  The device does not decode payloads:
 * the reference stops a COMBINED walk when decodeBuffer rejects an unsegmented payload
 * (:699-703) and skips the decrypt on assembly-state rejections (:744-818) -- its chain is out
 * of step with the sender's from there on anyway; the device decrypts every qualifying
 * section of a taken package.
 *
 * FPNN_AES_ERR_ARG: what fpnn_aes_udp_decrypt reports; unknown flags; PLAIN with b->in !=
 * b->out or b->out_off; non-NULL section inputs or nsections != 0 in u; data_keys NULL without
 * WALK_ONLY (recv) or at all (recv_take); max_pkgs == 0 or max_sections == 0, or a product
 * with b->count (recv_take: max_sections * ntake) above 32 bits; with b->count != 0, a NULL or
 * misaligned table (scan: 2 bytes; pkgs, sections: 4); with ntake != 0, NULL or misaligned
 * first_take or take.  FPNN_AES_ERR_KEYLEN for a 24-byte table.  conn_slot[j] >= slot_bound is
 * handled as by fpnn_aes_udp_decrypt.  Every value read from the caller's device tables
 * (first_dgram, first_take, take, and scan / pkgs / sections passed back in) is clamped
 * before it addresses memory; a breach (a table not monotone, a take entry out of range, one
 * that names no walked package or another connection's datagram, a package or section row
 * that leaves its datagram) decrypts nothing for that entry, leaves all other connections
 * exact, and makes the next fpnn_aes_engine_sync return FPNN_AES_ERR_DEVICE once.  Naming one
 * package twice is the caller's error: wrong plaintext, inside the datagrams' own bytes.
 *
 * nconn == 0 or b->count == 0 queues nothing (recv_take: also ntake == 0).  Both calls are
 * queued on the engine's stream with no host wait.  The data layer runs as max_sections
 * segments per datagram (recv) or per taken package (recv_take), empty where there is no
 * section to decrypt; after fpnn_aes_engine_reserve(max_segments, max_blocks) with
 * max_segments >= max(b->count, nconn, b->count * max_sections) for recv and
 * max_segments >= max(nconn, ntake * max_sections) for recv_take (max_blocks as for
 * fpnn_aes_udp_decrypt) they allocate nothing. */
#define FPNN_AES_UDP_F_WALK_ONLY 0x1u  /* package-decrypt and walk; no data decrypt, state untouched */
#define FPNN_AES_UDP_F_PLAIN     0x2u  /* b->out already holds package-plaintext (b->in == b->out): skip the package layer */

#define FPNN_AES_UDP_OK      0
#define FPNN_AES_UDP_SHORT   1 /* a length the reference's reads would leave */
#define FPNN_AES_UDP_VERSION 2 /* version byte above 2 */
#define FPNN_AES_UDP_TYPE    3 /* a package or component type the parser refuses (ECDH included) */
#define FPNN_AES_UDP_ACKS    4 /* ACKS bytes no multiple of 4 */
#define FPNN_AES_UDP_CLOSE   5 /* package only: ended at a CLOSE; accepted */
#define FPNN_AES_UDP_FULL    6 /* max_pkgs or max_sections reached */
#define FPNN_AES_UDP_LONG    7 /* datagram only: more than 65535 bytes */

typedef struct {       /* per datagram */
    uint16_t pkgs, sections;   /* rows used in the two tables */
    uint8_t  version, status;  /* FPNN_AES_UDP_* of the datagram as a whole */
    uint16_t reserved;         /* 0 */
} fpnn_aes_udp_scan;

typedef struct {       /* per package: the datagram itself, or each package included in an ARQ_ASSEMBLED one */
    uint32_t seq;              /* be32toh of header bytes 4..8 */
    uint8_t  type, flag, sign, status;
    uint16_t off, len;         /* the reference's _buffer and _bufferLength for this package, inside the datagram */
    uint16_t first_section, nsections;   /* into the datagram's row of the section table */
} fpnn_aes_udp_pkg;

typedef struct {       /* per component walked: DATA, ACKS, UNA, FORCESYNC, CLOSE, HEARTBEAT */
    uint8_t  type, flag;       /* a whole package's: the package's type and flag */
    uint16_t pkg;              /* index in the datagram's package row */
    uint16_t off, len;         /* payload inside the datagram; for segmented DATA, after packageId and index */
    uint16_t package_id, reserved;       /* segmented DATA: packageId; else 0 */
    uint32_t seg_index;        /* segmented DATA: the index; else 0 */
} fpnn_aes_udp_section;

int fpnn_aes_udp_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u, uint32_t flags,
                      uint32_t max_pkgs, uint32_t max_sections,
                      fpnn_aes_udp_scan *scan, fpnn_aes_udp_pkg *pkgs, fpnn_aes_udp_section *sections);
int fpnn_aes_udp_recv_take(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u,
                           uint32_t max_pkgs, uint32_t max_sections, const fpnn_aes_udp_scan *scan,
                           const fpnn_aes_udp_pkg *pkgs, const fpnn_aes_udp_section *sections,
                           const uint32_t *first_take, const uint32_t *take, uint32_t ntake);

/* ---- single call from host memory (the per-frame drop-in) --------------------------- */
/* Exactly rijndael_cfb_encrypt(ctx, encrypt, in, out, len, ivec, p_num)
 * (base/rijndael.c:1171-1201) with host buffers: stages through pinned memory,
 * runs the GPU kernels, copies back and updates ivec/p_num.  Synchronous. */
int fpnn_aes_cfb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt,
                      const uint8_t *in, uint8_t *out, size_t len, uint8_t ivec[16], size_t *p_num);

/* ---- the rest of rijndael.h, single calls from host memory (synchronous) ------------------ */
/* ECB: nblocks independent 16-byte blocks through the forward cipher (encrypt != 0,
 * ctx from fpnn_aes_setup_encrypt; rijndael_encrypt, base/rijndael.c:852-959) or the
 * inverse cipher (ctx from fpnn_aes_setup_decrypt; rijndael_decrypt, :961-1068).
 * in == out allowed. */
int fpnn_aes_ecb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt, const uint8_t *in, uint8_t *out,
                      size_t nblocks);
/* CBC exactly as rijndael_cbc_encrypt / _decrypt (base/rijndael.c:1070-1153): encrypt
 * zero-pads a partial last block and writes 16*ceil(len/16) bytes; decrypt reads
 * 16*ceil(len/16) bytes and writes len; ivec is updated to the last ciphertext block.
 * Decrypt takes the setup_decrypt schedule.  in == out allowed. */
int fpnn_aes_cbc_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt, const uint8_t *in, uint8_t *out,
                      size_t len, uint8_t ivec[16]);
/* OFB exactly as rijndael_ofb_encrypt (base/rijndael.c:1155-1169), (ivec, *p_num) carried. */
int fpnn_aes_ofb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, const uint8_t *in, uint8_t *out, size_t len,
                      uint8_t ivec[16], size_t *p_num);

/* ---- many frames from host memory (the cross-connection batch path, §8f row 1) ------- */
/* One entry per frame.  src/dst are host pointers (dst may equal src for in-place;
 * with FPNN_AES_F_WIRE_PREFIX, dst receives htole32(len) || ciphertext and must hold
 * len + 4 bytes and not overlap src).  key_slot indexes `keys`. */
typedef struct {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t len;
    uint32_t key_slot;
} fpnn_aes_host_frame;

/* Package-mode encrypt (encrypt != 0) or decrypt of n host frames: the frames are
 * gathered into pinned staging by a few host threads, and chunks are pipelined
 * (H2D of chunk i+1 || kernel of chunk i || D2H of chunk i-1) over the engine's
 * streams.  Results equal n PackageEncryptor calls.  Synchronous. */
int fpnn_aes_package_host(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                          const fpnn_aes_keyset *keys, uint32_t flags);

/* Stream-mode encrypt/decrypt of n host frames (StreamEncryptor::encrypt/decrypt,
 * core/Encryptor.cpp:53-70, one call per frame in the reference).  key_slot names the
 * stream: its key slot in `keys` AND its state (iv_state[16*slot .. +16], pos_state[slot],
 * host arrays of keys->count entries, StreamEncryptor::_iv/_pos), updated in place.  A
 * stream may appear many times: its frames are processed in array order, exactly as
 * that many successive calls.  Synchronous. */
int fpnn_aes_stream_host(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                         const fpnn_aes_keyset *keys, uint8_t *iv_state, uint32_t *pos_state);

/* fpnn_aes_stream_host for connections that live in a key table on the device: frames[i].key_slot
 * names the table slot, for the key (slot key_slot of `keys`) AND for the state, which stays
 * where fpnn_aes_stream_open wrote it: iv_state / pos_state are DEVICE arrays of slot_bound
 * entries (iv_state 16-byte aligned), read and updated by the kernels in place -- neither the
 * IV nor the state of such a connection is ever in host memory.  src / dst are host pointers
 * as above; frames in registered memory (fpnn_aes_host_register) take the host-mapped path,
 * others the staged one.  A slot may appear many times: its frames are processed in array
 * order, exactly as that many successive StreamEncryptor calls; a slot whose frames are all
 * empty keeps its state bit for bit, as do the slots the call does not name.  Synchronous, and
 * ordered behind work already queued on the engine's stream (an fpnn_aes_stream_open queued
 * just before it is seen).  The host knows every slot: a frame with key_slot >= slot_bound, or
 * slot_bound > fpnn_aes_keyset_capacity(keys), returns FPNN_AES_ERR_ARG before anything is
 * queued or touched; so do keys of another device and NULL or misaligned state arrays.  There
 * is no _multi form: a table lives on one device. */
int fpnn_aes_stream_host_at(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
        const fpnn_aes_keyset *keys, uint32_t slot_bound,
        uint8_t *iv_state /*dev*/, uint32_t *pos_state /*dev*/);

/* One host-frame batch over several engines -- e.g. one per GPU of the node, each
 * with its own copy of the key set (keys[k] created on engines[k], same count and key
 * length).  Package mode splits the frames into byte-balanced contiguous ranges; stream
 * mode gives whole streams (all frames of a key slot, in order) to engines, longest first
 * onto the least-loaded one.  Every engine runs its share through its own pipeline in
 * its own host thread; results are as from one call of fpnn_aes_package_host /
 * fpnn_aes_stream_host.  Synchronous. */
int fpnn_aes_package_host_multi(fpnn_aes_engine *const *engines, const fpnn_aes_keyset *const *keys, int n_engines,
                                int encrypt, const fpnn_aes_host_frame *frames, uint32_t n, uint32_t flags);
int fpnn_aes_stream_host_multi(fpnn_aes_engine *const *engines, const fpnn_aes_keyset *const *keys, int n_engines,
                               int encrypt, const fpnn_aes_host_frame *frames, uint32_t n, uint8_t *iv_state,
                               uint32_t *pos_state);

/* ---- host-mapped frames (zero-copy host-frame path) --------------------------------- */
/* Register [ptr, ptr + len) of host memory -- e.g. the arena a server allocates its
 * connections' socket buffers from -- with every GPU (hipHostRegister, portable + mapped;
 * the pages are locked).  fpnn_aes_package_host / _multi calls whose frames all lie in
 * registered memory (src: len bytes, dst: len (+4 with the wire prefix) bytes) are then
 * moved by the GPU itself over PCIe: no host gather/scatter and no pinned bounce copy;
 * the host threads only write 40 bytes of descriptor per frame.  A call whose frames
 * leave registered memory from frame k on runs frames [k, n) through the staged path;
 * calls that start outside it are staged entirely.  Ranges must not overlap; registration is process-wide.
 * Unregister only while no call uses the range. */
int fpnn_aes_host_register(void *ptr, size_t len);
int fpnn_aes_host_unregister(void *ptr);
/* 1 if [ptr, ptr + len) lies inside one registered range, else 0. */
int fpnn_aes_host_is_mapped(const void *ptr, size_t len);

/* ---- receive side: wire framing on the device (§8f row 3) --------------------------- */
/* Per received segment (the bytes one connection delivered), the outcome of walking its
 * frames: `frames` complete frames cover the first `consumed` bytes; the rest is an
 * incomplete frame to keep for the next call, unless status says the connection is bad. */
typedef struct {
    uint32_t frames;
    uint32_t status;   /* FPNN_AES_SCAN_* */
    uint64_t consumed;
} fpnn_aes_frame_scan;
#define FPNN_AES_SCAN_OK         0 /* stopped at the end of the data (maybe mid-frame) */
#define FPNN_AES_SCAN_FULL       1 /* max_frames frames recorded; call again from `consumed` */
#define FPNN_AES_SCAN_TOO_LARGE  2 /* frame above max_len: the reference closes the connection */
#define FPNN_AES_SCAN_BAD_MAGIC  3 /* stream: header magic is not "FPNN" */
#define FPNN_AES_SCAN_BAD_MTYPE  4 /* stream: mtype not 0/1/2 (FPMessage::BodyLen throws) */
#define FPNN_AES_SCAN_BAD_LENGTH 5 /* stream: message length <= 0 by the reference's int arithmetic */

/* Package-mode receive: EncryptedPackageReceiver::recvPackage + fetch
 * (core/EncryptedPackageReceiver.cpp:60-118) for many connections at once.  Segment i of
 * b (b->in + in_off[i], len_i bytes, key slot slot_i) starts at a frame boundary and holds
 * [htole32(n)][n bytes ciphertext] wire frames.  The complete frames' bodies are
 * decrypted (fresh chain each, like PackageEncryptor::decrypt) to b->out at the same
 * offsets (b->out_off must be NULL; in place when b->out == b->in); prefixes and the
 * trailing incomplete frame are not written.  Frame j of segment i is reported at
 * [i*max_frames + j]: frame_off = body offset within the segment, frame_len = n
 * (dev arrays; scan[count] dev).  max_len: Config::_max_recv_package_length (8 MiB). */
int fpnn_aes_package_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint32_t max_len, uint32_t max_frames,
                          uint64_t *frame_off, uint32_t *frame_len, fpnn_aes_frame_scan *scan);

/* Stream-mode receive: EncryptedStreamReceiver (core/EncryptedStreamReceiver.cpp:72-163).
 * Segment i is the ciphertext newly received on stream i; it is decrypted exactly as
 * fpnn_aes_stream_decrypt (state advanced over every byte) and the plaintext, preceded
 * by carry[i] bytes already in b->out (the previous call's incomplete message, NULL = 0),
 * is split into FPNN messages: 12-byte header + FPMessage::BodyLen (proto/FPMessage.cpp:27-44).
 * frame_off is relative to the region start (out + out_off[i] - carry[i]), frame_len is the
 * whole message length (what fetch() hands to the decoder). */
int fpnn_aes_stream_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state,
                         const uint32_t *carry, uint32_t max_len, uint32_t max_frames, uint64_t *frame_off,
                         uint32_t *frame_len, fpnn_aes_frame_scan *scan);
/* The same with segment i's state AND key at slot state_slot[i] (b->key_slot NULL; the
 * state arrays hold slot_bound entries; the contracts of fpnn_aes_stream_decrypt_frames_at
 * with one frame per stream).  carry, the frame tables and scan stay per segment. */
int fpnn_aes_stream_recv_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *state_slot,
                            uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state, const uint32_t *carry,
                            uint32_t max_len, uint32_t max_frames, uint64_t *frame_off, uint32_t *frame_len,
                            fpnn_aes_frame_scan *scan);

/* ---- memory on an engine's device, for callers built without HIP headers ------------ */
/* (StreamReceiverBatch uses these: libfpnn_aes.so itself has no HIP dependency, see the
 * library layout note at the top.)  device_free waits for the device; copy_async queues a
 * copy of `bytes` between any two of host-pinned / device memory on the engine stream. */
int fpnn_aes_device_alloc(fpnn_aes_engine *e, size_t bytes, void **out);
int fpnn_aes_device_free(fpnn_aes_engine *e, void *p);
int fpnn_aes_pinned_alloc(fpnn_aes_engine *e, size_t bytes, void **out);
int fpnn_aes_pinned_free(fpnn_aes_engine *e, void *p);
int fpnn_aes_copy_async(fpnn_aes_engine *e, void *dst, const void *src, size_t bytes);

/* NUMA placement of the engine's host side: `node` the node its pinned
 * arenas (pinned_alloc, the host-frame staging) are allocated on and its copy threads run
 * on (-1: none); `device_node` the GPU's node from sysfs (-1: unknown); `ncpus` the node's
 * CPUs the copy threads are pinned to (0: unpinned).  fpnn_aes_last_error() then holds one
 * line saying how the placement was chosen.  FPNN_AES_NUMA=auto|off|<node>. */
int fpnn_aes_engine_numa(fpnn_aes_engine *e, int *node, int *device_node, int *ncpus);

/* ---- synthetic data (bench/tests utility, not part of the cipher) ------------------ */
/* dst[k] = byte (off+k)&7 of splitmix64((off+k)>>3 + seed*0xD1B54A32D192ED03), LE. */
int fpnn_aes_fill_synthetic(fpnn_aes_engine *e, uint8_t *dst, uint64_t nbytes, uint64_t seed,
                            uint64_t byte_offset);

/* ---- instrumentation ---------------------------------------------------------------- */
/* When enabled, every batch call records HIP events around its main kernel on the
 * engine stream; fpnn_aes_engine_kernel_stats returns the count and summed milliseconds
 * of the main-kernel launches since the last reset (synchronizes the stream). */
int fpnn_aes_engine_set_timing(fpnn_aes_engine *e, int enable);
int fpnn_aes_engine_kernel_stats(fpnn_aes_engine *e, int which /* FPNN_AES_K_* */, uint64_t *launches,
                                 double *total_ms);
int fpnn_aes_engine_reset_stats(fpnn_aes_engine *e);
/* Name of the kernel variant the last call queued as its main kernel for that direction
 * ("cfb_decrypt_dense", "cfb_encrypt_queue", ...; "" before any call).  Static storage. */
const char *fpnn_aes_engine_last_kernel(fpnn_aes_engine *e, int which);
#define FPNN_AES_K_DECRYPT 0
#define FPNN_AES_K_ENCRYPT 1
#define FPNN_AES_K_HOST 2 /* last_kernel only: the last host-frame call's path, "host_mapped",
                           "host_staged" or "host_mapped+staged" */

/* Version string of the built library (kernel variant + build flags). */
const char *fpnn_aes_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FPNN_AES_H */
