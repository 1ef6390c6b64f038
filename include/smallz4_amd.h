/* smallz4_amd.h -- C ABI of the MI355X (gfx950) LZ4 optimal-parse compressor.
 *
 * Drop-in boundary for the reference's compression entry point
 *   smallz4::lz4(GET_BYTES, SEND_BYTES, maxChainLength, dictionary,
 *                useLegacyFormat, userPtr)          reference smallz4.h:47-64
 * Everything here is plain C: pointers, sizes, integer status codes.  The C++
 * mirror of the reference class (include/smallz4_amd.hpp) and the Python
 * package (smallz4_amd/) are thin layers over these symbols.
 *
 * Compression levels are the reference's maxChainLength (smallz4.cpp:175-239):
 *   0 stored, 1..3 greedy, 4..6 lazy + optimal parse, 7..65534 optimal parse
 *   with a chain limit, 65535 ("-9") unlimited optimal parse.
 * Output is byte-identical to the reference at the same level.
 */
#ifndef SMALLZ4_AMD_H
#define SMALLZ4_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define SZ4_OK              0
#define SZ4_E_ARG          -1  /* bad argument                                  */
#define SZ4_E_DEVICE       -2  /* HIP runtime error                             */
#define SZ4_E_CAPACITY     -3  /* output buffer too small                       */
#define SZ4_E_NOMEM        -4  /* device/host allocation failed                 */
#define SZ4_E_UNSUPPORTED  -5  /* reserved: every level, format and dictionary is supported */
#define SZ4_E_CORRUPT      -6  /* decoder: a frame the reference decoder rejects           */

/* frame header written by sz4_compress_blocks_device */
#define SZ4_HEADER_SMALLZ4     0  /* exactly smallz4's header: 04 22 4D 18 40 70 DF  */
#define SZ4_HEADER_INDEPENDENT 1  /* LZ4 frame flagged block-independent, BD sized   */
#define SZ4_HEADER_NONE        2  /* no header and no end mark: bare blocks          */

typedef struct sz4_ctx sz4_ctx;

/* Version of the reference interface mirrored (smallz4.h:67-70). */
const char* sz4_version(void);

/* Create a compression context bound to HIP device `device`.  Scratch space is
 * allocated lazily and grown on demand; `reserve_bytes` pre-sizes it for that
 * much input (0 = on first use).  A context serves one call at a time: threads
 * that compress concurrently use a context each.  Every call makes the
 * context's device current and restores the caller's current device. */
int sz4_create(sz4_ctx** ctx, int device, uint64_t reserve_bytes);
void sz4_destroy(sz4_ctx* ctx);

/* Process-wide context pool (thread-safe): sz4_acquire hands out an idle context of `device` (creating
 * one when all are busy), sz4_release returns it.  Concurrent callers get different contexts, so
 * calls through the pool are reentrant -- the reference builds a fresh object per call
 * (smallz4.h:56-64).  Pooled contexts live until the process exits; one returned holding more device
 * memory than sz4_set_pool_cap is trimmed first. */
int sz4_acquire(sz4_ctx** ctx, int device);
void sz4_release(sz4_ctx* ctx);

/* Worst-case frame size for n input bytes cut into blocks of block_size. */
uint64_t sz4_bound(uint64_t n, uint32_t block_size);

/* Compress n bytes already resident in device memory as independent blocks of
 * block_size bytes (last block shorter).  Each block's bytes in the output
 * (4-byte size word + payload) are exactly what smallz4::lz4 emits for that
 * block compressed on its own (reference smallz4.h:476-813 with one block).
 * Any n in bounded memory: the blocks are compressed in pieces of at most
 * sz4_set_batch_chunk bytes (by default 448 MiB, split into equal pieces, and capped so that the scratch -- under 50 bytes
 * per piece byte -- takes at most a quarter of the device memory the context could use now;
 * under a sz4_set_device_limit bound about 1/64 of the bound).  A piece whose scratch cannot
 * be allocated is halved and retried, down to 16 MiB, before SZ4_E_NOMEM: the context first releases the
 * device buffers it holds (all but a live queue's), so a retry succeeds wherever a new context would, and a
 * call that succeeds after retries leaves sz4_last_error empty.
 *
 *   d_in, d_out   device pointers (d_out capacity out_cap bytes)
 *   block_size    1 .. 4 MiB
 *   max_chain     reference maxChainLength (0..65535)
 *   header        SZ4_HEADER_*
 *   out_size      host pointer, receives the frame size
 *   stream        hipStream_t (NULL = default stream); the call returns after
 *                 the stream has finished (out_size needs the result)
 */
int sz4_compress_blocks_device(sz4_ctx* ctx, const void* d_in, uint64_t n, uint32_t block_size,
                               uint32_t max_chain, int header, void* d_out, uint64_t out_cap,
                               uint64_t* out_size, void* stream);

/* Per-block result sizes of the last sz4_compress_blocks_device call
 * (4-byte word included), copied to host array sizes[0..nblocks).  Returns the
 * number of blocks, or a negative status. */
int64_t sz4_last_block_sizes(sz4_ctx* ctx, uint32_t* sizes, uint64_t max_blocks);

/* ---- ragged batch: many separate buffers of different sizes ------------------------------------
 * Worst-case output of sz4_compress_batch_device: the sum over the items of (size + 4) -- stored blocks
 * are never larger than their input. */
uint64_t sz4_batch_bound(const uint32_t* sizes, uint64_t count);

/* Compress `count` separate device buffers, each 0 .. 4 MiB, each as one LZ4 block on its own: item i's
 * output (4-byte size word + payload, the word's top bit set when the item is stored) is exactly what
 * smallz4::lz4 emits for that buffer alone; an empty item produces no bytes.  The blocks land back to
 * back in d_out in caller order, as bare blocks (what SZ4_HEADER_NONE writes).  The items are staged by
 * one gather kernel per internal piece (any source alignment; nothing is read outside the aligned
 * 16-byte words that overlap an item) and compressed in pieces of whole items: at most
 * sz4_set_batch_chunk bytes (capped and retried as in sz4_compress_blocks_device) and at most 32768
 * items each.  Items above 64 KiB are compressed in a pipeline run of their own inside their piece, so
 * one large item does not slow the small ones down.  No dictionary, no linked items.
 *
 *   in_ptrs      HOST array of count DEVICE pointers (may be NULL where the size is 0)
 *   in_sizes     HOST array of count sizes; one above 4 MiB: SZ4_E_ARG before any work
 *   max_chain    reference maxChainLength (0..65535)
 *   d_out        device pointer; out_cap < sz4_batch_bound: SZ4_E_CAPACITY before any work
 *   out_offsets  HOST array of count + 1: item i occupies d_out[out_offsets[i], out_offsets[i + 1])
 *   stream       hipStream_t (NULL = default stream); the call returns after the stream has finished
 * sz4_last_block_sizes then reports one size per item (0 for an empty item), in caller order. */
int sz4_compress_batch_device(sz4_ctx* ctx, const void* const* in_ptrs, const uint32_t* in_sizes, uint64_t count,
                              uint32_t max_chain, void* d_out, uint64_t out_cap, uint64_t* out_offsets,
                              void* stream);

/* Device time (milliseconds) of the gather kernels of the last sz4_compress_batch_device call (with
 * sz4_set_timing on; it is not part of any sz4_last_stage_ms stage). */
float sz4_last_gather_ms(sz4_ctx* ctx);

/* The reverse: item i is the bare block d_blocks[offsets[i], offsets[i + 1]) (HOST array of count + 1;
 * a non-empty item is its 4-byte size word + payload) and decodes to d_out[out_offsets[i],
 * out_offsets[i + 1]) (HOST array of count + 1) -- exactly what the reference decoder gives for a frame
 * holding that block alone.  Items are independent: a match that reaches below its item's first output
 * byte reads zeros (the reference's zero-initialised history), never another item's output.  One
 * wavefront decodes one item.
 * d_out == NULL / out_cap == 0 queries the sizes: out_offsets is filled and SZ4_E_CAPACITY returned, as
 * sz4_unlz4 does.  SZ4_E_CORRUPT: an item whose size word disagrees with its extent, a non-empty item
 * shorter than 4 bytes, a malformed block (see sz4_unlz4). */
int sz4_unlz4_batch_device(sz4_ctx* ctx, const void* d_blocks, const uint64_t* offsets, uint64_t count,
                           void* d_out, uint64_t out_cap, uint64_t* out_offsets, void* stream);

/* ---- typed items: the byte-plane split (Parquet's BYTE_STREAM_SPLIT, Blosc's and HDF5's "shuffle") ----
 * An item of n bytes holding elements of width E (1, 2, 4 or 8) has m = n / E whole elements and n % E tail
 * bytes; its split is
 *     split[k * m + e] = item[e * E + k]   (0 <= k < E, 0 <= e < m)
 *     split[E * m + j] = item[E * m + j]   (the tail, unchanged, after the planes)
 * (the identity for E = 1 and for n < E).  smallz4_amd/planes.py states both directions in numpy.
 *
 * As sz4_compress_batch_device; item i is split by elem_sizes[i] (HOST array of count, each 1, 2, 4 or 8;
 * anything else: SZ4_E_ARG before any work) while it is staged, at no extra pass over the data.  Item i's
 * output is exactly what smallz4::lz4 emits for split(item i) on its own: an ordinary LZ4 block that any
 * decoder reads, giving the split bytes.  Widths are per item; with all widths 1 the call is the plain call.
 * sz4_batch_bound, out_offsets, sz4_last_block_sizes and the pieces are unchanged, and sz4_last_gather_ms
 * covers the splitting gather. */
int sz4_compress_batch_typed_device(sz4_ctx* ctx, const void* const* in_ptrs, const uint32_t* in_sizes,
                                    const uint8_t* elem_sizes, uint64_t count, uint32_t max_chain, void* d_out,
                                    uint64_t out_cap, uint64_t* out_offsets, void* stream);

/* As sz4_unlz4_batch_device; item i's decoded bytes are merged (the inverse of the split) by elem_sizes[i]
 * on their way to d_out, so d_out[out_offsets[i], out_offsets[i + 1]) is the original item.  d_out may have
 * any alignment; an item that lands at a multiple of its element width is merged with 16-byte stores and
 * byte permutes, any other byte by byte.  The blocks decode into a buffer of the context (the decoded
 * bytes once more, counted by sz4_device_bytes, released by sz4_trim).  Same query mode, same error codes;
 * a width other than 1, 2, 4 or 8: SZ4_E_ARG before any work. */
int sz4_unlz4_batch_typed_device(sz4_ctx* ctx, const void* d_blocks, const uint64_t* offsets,
                                 const uint8_t* elem_sizes, uint64_t count, void* d_out, uint64_t out_cap,
                                 uint64_t* out_offsets, void* stream);

/* Device time (milliseconds) of the merge kernel of the last sz4_unlz4_batch_typed_device call (with
 * sz4_set_timing on; 0 when every width was 1). */
float sz4_last_merge_ms(sz4_ctx* ctx);

/* ---- filtered items: the bit-plane shuffle (the "bitshuffle" of HDF5 and Blosc) beside the byte-plane split ----
 * LZ4 has no entropy stage: a byte plane of a few frequent values gains nothing, a constant BIT plane is a run.
 * An item of n bytes and element width E (1, 2, 4 or 8) has m = n / E whole elements, of which g = m - m % 8 are
 * shuffled into 8 * E bit rows of G = g / 8 bytes each (bits numbered from the least significant):
 *     bit (e & 7) of shuf[(8 * k + b) * G + (e >> 3)] = bit b of item[e * E + k]   (0 <= k < E, 0 <= b < 8, 0 <= e < g)
 *     shuf[j] = item[j]                                                            (g * E <= j < n)
 * -- the byte-plane split of the first g elements with every plane bit-transposed into its 8 rows; the m % 8
 * left-over elements and the n % E tail bytes keep their place after the rows.  It changes no size, is the
 * identity for g = 0 (n < 8 * E), and E = 1 is meaningful (the bit rows of the bytes).  smallz4_amd/planes.py
 * states both directions in numpy (bit_split, bit_merge). */
#define SZ4_FILTER_BYTES 0 /* the byte-plane split: what the typed calls do */
#define SZ4_FILTER_BITS 1  /* the bit-plane shuffle above                   */

/* As sz4_compress_batch_typed_device with a filter per item: filters is a HOST array of count bytes, each
 * SZ4_FILTER_BYTES or SZ4_FILTER_BITS.  filters == NULL, or SZ4_FILTER_BYTES throughout, is exactly the typed call
 * (same code path, same bytes).  Any other filter value, or a width other than 1, 2, 4 or 8: SZ4_E_ARG before
 * any device work, nothing written.  Item i's block is exactly what smallz4::lz4 emits for the filtered item on
 * its own -- for SZ4_FILTER_BITS shuf(item i, E_i) -- an ordinary LZ4 block that any decoder reads, giving the
 * filtered bytes.  The shuffle happens while the item is staged, at no extra pass over the data; a batch whose
 * widths are all 1 but which has a SZ4_FILTER_BITS item is not the plain call.  sz4_batch_bound, out_offsets,
 * sz4_last_block_sizes, the pieces and sz4_last_gather_ms are as in the typed call. */
int sz4_compress_batch_filtered_device(sz4_ctx* ctx, const void* const* in_ptrs, const uint32_t* in_sizes,
                                       const uint8_t* elem_sizes, const uint8_t* filters, uint64_t count,
                                       uint32_t max_chain, void* d_out, uint64_t out_cap, uint64_t* out_offsets,
                                       void* stream);

/* As sz4_unlz4_batch_typed_device with a filter per item (filters as above; NULL or SZ4_FILTER_BYTES throughout is
 * exactly the typed call): item i's decoded bytes pass through the inverse of its filter on their way to d_out.
 * d_out may have any alignment; a SZ4_FILTER_BITS item is unshuffled 8 elements at a time with 16-byte stores
 * where it lands at a multiple of 8 (E = 1), 16 (E = 2), 32 (E = 4) or 64 (E = 8) bytes, counted from the 16-byte
 * boundary at or below d_out, and bit by bit elsewhere.  Same query mode, same error codes, sz4_last_merge_ms as in the typed call. */
int sz4_unlz4_batch_filtered_device(sz4_ctx* ctx, const void* d_blocks, const uint64_t* offsets,
                                    const uint8_t* elem_sizes, const uint8_t* filters, uint64_t count, void* d_out,
                                    uint64_t out_cap, uint64_t* out_offsets, void* stream);

/* ---- decode queue: the batch decoders as an enqueue, nothing on the host ---------------------------------
 * sz4_unlz4_batch_device takes host tables, waits for the stream twice and fails as a whole on one bad item.
 * A decode queue takes DEVICE tables, writes per-item sizes and statuses on the device and only launches:
 * sz4_dq_enqueue never synchronises, never allocates and never copies between host and device, and issues one
 * chain of kernels on `stream` (no fork), so it can be captured in a HIP graph and replayed.
 *
 * sz4_dq_create reserves once what an enqueue of up to max_items items (1 .. 65536; else SZ4_E_ARG) holding up
 * to max_src_bytes of blocks needs: a record per item and the sequence lists (about 5.4 bytes per source byte).
 * The scratch belongs to the context: sz4_device_bytes counts it and sz4_set_device_limit bounds it (over the
 * bound: SZ4_E_NOMEM), but neither a call that sheds buffers under the bound nor sz4_trim releases it while
 * the queue lives -- a captured graph holds its addresses.  Destroy a queue before its context, and only after
 * the last graph captured from it is gone and its last enqueue has finished.
 * A queue serves one stream at a time: enqueues on one stream are ordered by the stream; using a queue from
 * two streams needs the caller's own event between them.  An enqueue does not count as a call on the context
 * (sz4_last_error is not touched); other calls on the context may run between enqueues. */
typedef struct sz4_dq sz4_dq;

/* per-item status, written to d_status */
#define SZ4_ITEM_OK        0
#define SZ4_ITEM_CORRUPT   1  /* what sz4_unlz4_batch_device answers SZ4_E_CORRUPT for */
#define SZ4_ITEM_CAPACITY  2  /* decoded size > dst cap; d_out_sizes holds the size needed */
#define SZ4_ITEM_ARG       3  /* width not 1/2/4/8, or a null pointer with a non-zero size/cap needed */
#define SZ4_ITEM_QUEUE     4  /* the batch's source bytes exceed the queue's max_src_bytes at this item */
#define SZ4_ITEM_INTERNAL  5  /* second pass decoded a different length than the size pass (compress queue: below) */

int sz4_dq_create(sz4_ctx* ctx, uint32_t max_items, uint64_t max_src_bytes, sz4_dq** q);
void sz4_dq_destroy(sz4_dq* q);

/* Every d_ array is DEVICE memory of `count` entries, read (and written) when the kernels run, not when the
 * call is made: a captured enqueue replayed after the caller rewrote the tables decodes the new tables.
 *   d_src, d_src_sizes  item i is the bare block [d_src[i], d_src[i] + d_src_sizes[i]): size word + payload,
 *                       exactly an item of sz4_unlz4_batch_device.  Any alignment, separate allocations;
 *                       nothing is read outside the aligned 16-byte words that overlap an item
 *   d_dst, d_dst_caps   it decodes to [d_dst[i], d_dst[i] + d_out_sizes[i]), any alignment; no store lands at or
 *                       beyond d_dst[i] + d_dst_caps[i], nor beyond d_dst[i] + the decoded size
 *   d_elems             element width per item (1, 2, 4 or 8), or NULL: every width 1.  For a width E > 1 the
 *                       result is the merge of the decoded planes, what sz4_unlz4_batch_typed_device gives --
 *                       the decoder stores every byte at its merged place, there is no second pass
 *   d_out_sizes         decoded bytes per item (0 for a failed item, the size needed for SZ4_ITEM_CAPACITY)
 *   d_status            SZ4_ITEM_* per item
 * The decoded bytes are those of sz4_unlz4_batch_device / _typed_device for that item (zero history, items
 * never see each other).  A size-0 item gives size 0 and SZ4_ITEM_OK, and neither of its pointers is looked
 * at.  An item whose status is not SZ4_ITEM_OK has no byte of its destination written; the other items decode
 * normally.  Items whose running source bytes pass max_src_bytes, from the first such item on, get
 * SZ4_ITEM_QUEUE.  One wavefront decodes one item.
 * Returns SZ4_OK once enqueued; SZ4_E_ARG before any device work for a null queue or table (d_elems may be
 * NULL) or count > max_items; SZ4_E_DEVICE for a launch error. */
int sz4_dq_enqueue(sz4_dq* q, const void* const* d_src, const uint32_t* d_src_sizes, void* const* d_dst,
                   const uint32_t* d_dst_caps, const uint8_t* d_elems, uint32_t count, uint32_t* d_out_sizes,
                   uint32_t* d_status, void* stream);

/* ---- compress queue: sz4_compress_batch_typed_device as an enqueue, nothing on the host --------------------
 * The batch compressors plan, allocate, upload and wait on every call.  A compress queue fixes the item count,
 * the item sizes and element widths and the level when it is created; the sources, the output and the result
 * tables are device memory read and written when the kernels run.  sz4_cq_enqueue never synchronises, never
 * allocates and never copies between host and device, and issues one chain of kernels on `stream`
 * (no fork), so it can be captured in a HIP graph and replayed.  Its result tables are by construction the
 * d_src / d_src_sizes of sz4_dq_enqueue: a compress -> decode round trip needs no host step in between.
 *
 * Limits, all checked by sz4_cq_create before any device work (SZ4_E_ARG, *q = NULL):
 *   count       1 .. 32768 items
 *   sizes       at most 4 MiB each (0: an empty item, which has no block); widths 1, 2, 4 or 8
 *   max_chain   0 or 7 .. 65535.  Levels 1 .. 6 (greedy / lazy) settle their shortcut intervals in rounds
 *               that read a status word on the host, and so does dictionary mode: neither is available here
 *   staged      the sum of the sizes, each rounded up to 64, is at most 448 MiB
 * One kind of item is advised: when an item does not fit the match finders' LDS (more than 65541 bytes) every
 * item of the queue runs through the finders that read their window from HBM -- the bytes are the same, the
 * small items are slower.  The synchronous calls split such a set into two runs; a queue does not.
 *
 * sz4_cq_create plans the run, reserves everything an enqueue names -- about 50 bytes per staged byte plus
 * 16 KiB per item -- uploads the plan and waits once.  The scratch belongs to the context: sz4_device_bytes
 * counts it and sz4_set_device_limit bounds it (over the bound: SZ4_E_NOMEM, nothing left allocated), but
 * neither a call that sheds buffers under the bound nor sz4_trim releases it while the queue lives -- a captured
 * graph holds its addresses.  It is the queue's own: other calls on the context, compressor calls included,
 * may run between enqueues.  Destroy a queue before its context, and only after the last graph captured from it
 * is gone and its last enqueue has finished.
 * A queue serves one stream at a time: enqueues on one stream are ordered by the stream; using a queue from
 * two streams needs the caller's own event between them.  An enqueue does not count as a call on the context
 * (sz4_last_error is not touched); sz4_set_timing and sz4_debug_stop_after do not apply to it. */
typedef struct sz4_cq sz4_cq;

/* sizes[count], elem_sizes[count] (NULL: every width 1) are HOST arrays, copied. */
int sz4_cq_create(sz4_ctx* ctx, const uint32_t* sizes, const uint8_t* elem_sizes, uint32_t count,
                  uint32_t max_chain, sz4_cq** q);
void sz4_cq_destroy(sz4_cq* q);
/* == sz4_batch_bound(sizes, count); 0 for a null queue */
uint64_t sz4_cq_bound(const sz4_cq* q);

/*   d_src          DEVICE table of `count` device addresses, read when the kernels run: a captured enqueue
 *                  replayed after the table was rewritten compresses the new buffers.  Any alignment; nothing
 *                  is read outside the aligned 16-byte words that overlap an item.  The entry of an empty item
 *                  is not looked at.  A null entry of a non-empty item is never dereferenced: the item is
 *                  compressed as zeros and its status is SZ4_ITEM_ARG
 *   d_out, out_cap the output and its size, passed BY VALUE: a captured enqueue writes the same buffer on every
 *                  replay.  out_cap < sz4_cq_bound(q): SZ4_E_CAPACITY before any device work.  No store lands
 *                  at or beyond d_out + sz4_cq_bound(q)
 *   d_block_ptrs, d_block_sizes, d_status   device tables of `count` entries, written by the kernels: the
 *                  address of item i's bare block inside d_out, its length (size word included, stored flag
 *                  masked off; 0 for an empty item, whose address is where the next block starts), and
 *                  SZ4_ITEM_OK, SZ4_ITEM_ARG or SZ4_ITEM_INTERNAL.  SZ4_ITEM_INTERNAL is given to every item,
 *                  with size 0, when a capacity invariant of the pipeline failed (SZ4_E_DEVICE from the
 *                  synchronous calls)
 *   d_total        device uint64_t receiving the bytes written to d_out (the sum of the sizes), or NULL
 * The blocks lie back to back in caller order and are byte for byte those of sz4_compress_batch_typed_device
 * on the same items: the reference's block of split(item, width).
 * Returns SZ4_OK once enqueued; SZ4_E_ARG for a null queue, d_src, d_out or result table; SZ4_E_DEVICE for a
 * launch error. */
int sz4_cq_enqueue(sz4_cq* q, const void* const* d_src, void* d_out, uint64_t out_cap, uint64_t* d_block_ptrs,
                   uint32_t* d_block_sizes, uint32_t* d_status, uint64_t* d_total, void* stream);

/* ---- sized compress queue: the item sizes come from a device table at every enqueue ---------------------------
 * As sz4_cq_create, but caps[i] is the LARGEST size item i may have at an enqueue (0 .. 4 MiB; an item of
 * capacity 0 is always empty).  The limits are sz4_cq_create's, applied to the capacities, and
 * sz4_cq_bound(q) == sz4_batch_bound(caps, count).  Every item keeps a fixed slot of the scratch, laid out for
 * its capacity; sz4_cq_destroy serves both kinds of queue.  The SZ4_DP_SIZE tuning knob does not apply. */
int sz4_cq_create_sized(sz4_ctx* ctx, const uint32_t* caps, const uint8_t* elem_sizes, uint32_t count,
                        uint32_t max_chain, sz4_cq** q);

/* As sz4_cq_enqueue, plus d_src_sizes: a DEVICE table of `count` sizes, read when the kernels run -- a captured
 * enqueue replayed after the table was rewritten compresses the new sizes.  With n = d_src_sizes[i], item i gives
 *   0 < n <= caps[i]   exactly the block sz4_compress_batch_typed_device writes for the n bytes at d_src[i] with
 *                      width elem_sizes[i] (the reference's block of split(item[:n], width)); SZ4_ITEM_OK.
 *                      A null d_src[i] is never dereferenced: n zeros are compressed, SZ4_ITEM_ARG
 *   n == 0             no bytes: size 0 at the address where the next block starts; d_src[i] is not looked at;
 *                      SZ4_ITEM_OK
 *   n > caps[i]        as an empty item, the source is not read; SZ4_ITEM_CAPACITY
 * Blocks lie back to back in caller order, d_total is their sum, and no store lands at or beyond
 * d_out + sz4_cq_bound(q).  SZ4_ITEM_INTERNAL keeps its meaning.  Everything else said of sz4_cq_enqueue
 * holds: kernel launches only (no memset, copy, wait or allocation), one chain on one stream, not a call on
 * the context.  The launches and their grids are those of the capacities, whatever the sizes: an enqueue of
 * small sizes costs the launch slots of the full capacities (a wavefront that finds its entry unused returns
 * at once), plus one small kernel that re-derives the plan.
 * sz4_cq_enqueue on a sized queue, sz4_cq_enqueue_sized on a queue of sz4_cq_create, and a null d_src_sizes
 * return SZ4_E_ARG before any device work. */
int sz4_cq_enqueue_sized(sz4_cq* q, const void* const* d_src, const uint32_t* d_src_sizes, void* d_out,
                         uint64_t out_cap, uint64_t* d_block_ptrs, uint32_t* d_block_sizes, uint32_t* d_status,
                         uint64_t* d_total, void* stream);

/* Whole-stream compression with the exact semantics of
 * smallz4::lz4(getBytes, sendBytes, maxChainLength, dictionary, useLegacyFormat)
 * (reference smallz4.h:47-64): 4 MiB dependent blocks (8 MiB independent
 * blocks in legacy format), optional dictionary, identical output bytes.
 * Host buffers; the device does all compression work, chunk by chunk as in
 * sz4_lz4_stream (fixed device footprint). */
int sz4_lz4(sz4_ctx* ctx, const void* in, uint64_t n, uint32_t max_chain, const void* dict,
            uint64_t dict_len, int legacy, void* out, uint64_t out_cap, uint64_t* out_size);

/* Worst-case size of sz4_lz4's output. */
uint64_t sz4_lz4_bound(uint64_t n, int legacy);

/* The reference's callback types (smallz4.h:41-44): read up to numBytes into data (0 = end of
 * input); write numBytes from data. */
typedef size_t (*sz4_get_bytes)(void* data, size_t numBytes, void* userPtr);
typedef void (*sz4_send_bytes)(const void* data, size_t numBytes, void* userPtr);

/* smallz4::lz4(getBytes, sendBytes, maxChainLength, dictionary, useLegacyFormat, userPtr)
 * (reference smallz4.h:47-64, 476-813) in bounded memory: the input is pulled through get_bytes
 * (64 KiB per call, as the reference's BufferSize) and compressed in chunks of whole 4 MiB blocks
 * (8 MiB legacy) -- sz4_set_stream_chunk bytes per chunk, 64 MiB by default -- each chunk carrying
 * the previous one's last 64 KiB and chain state, so the output is byte-identical to one pass over
 * the whole input and the device footprint does not grow with the input.  send_bytes receives the
 * header, then per block four 1-byte calls for the size word followed by the payload, then the end
 * mark: the reference's call pattern (smallz4.h:478-496, 770-780, 807-812).  Both callbacks run on
 * the calling thread; the GPU compresses chunk i+1 while chunk i is sent and chunk i+2 is read and
 * uploaded (three HIP streams).  Pinned host buffers grow with the input up to one chunk.
 * A context serves one call at a time (use one context per thread). */
int sz4_lz4_stream(sz4_ctx* ctx, sz4_get_bytes get_bytes, sz4_send_bytes send_bytes, uint32_t max_chain,
                   const void* dict, uint64_t dict_len, int legacy, void* user);

/* Input bytes per chunk of the stream paths (sz4_lz4_stream, sz4_lz4; sz4_unlz4_stream queues half
 * as many frame bytes); rounded down to whole blocks, at least one.  0 restores the 64 MiB default. */
void sz4_set_stream_chunk(sz4_ctx* ctx, uint64_t bytes);

/* Input bytes per internal piece of sz4_compress_blocks_device and sz4_compress_batch_device (whole
 * blocks / items, at least one); the
 * device scratch is about 36-50 bytes per piece byte.  An explicit size is not capped by free memory.
 * 0 restores the default (448 MiB, capped by free memory). */
void sz4_set_batch_chunk(sz4_ctx* ctx, uint64_t bytes);

/* Device time (milliseconds) of each pipeline stage of the last call, measured
 * with HIP events on the call's stream.  stage_ms[0..n) receives
 * {runs, sort, find_sorted, find_long, parse, assemble} (find_sorted is the
 * k_find_sorted kernel alone); returns the number of stages. */
int sz4_last_stage_ms(sz4_ctx* ctx, float* stage_ms, int n);

/* Enable (1) or disable (0) per-stage event timing (default off). */
void sz4_set_timing(sz4_ctx* ctx, int on);

/* Diagnostics: stop the pipeline after stage `stop_after` (0 = run everything,
 * 3 = after the match search, 4 = after the parse) on subsequent calls, and copy
 * the per-position match arrays of the last call (length u32, distance u16, one
 * entry per input byte) to host memory.  After stage 4 at levels > 3 the lengths
 * are the parse's choices (1 = literal).  Used by the intermediate parity tests. */
void sz4_debug_stop_after(sz4_ctx* ctx, int stop_after);
int sz4_debug_matches(sz4_ctx* ctx, uint32_t* len, uint16_t* dist, uint64_t n);
/* The same copy, but always of the match arrays themselves: at levels > 3 what the parse was given
 * (at levels 4..6 after the greedy/lazy skip bookkeeping), whatever stage the run stopped after. */
int sz4_debug_parse_input(sz4_ctx* ctx, uint32_t* len, uint16_t* dist, uint64_t n);
/* Diagnostics of the device memory accounting, for the tests of the out-of-memory paths: out[0] = buffer
 * growths that reached the allocator since the context was created, out[1] = growths an injected failure
 * hit (the test hooks SZ4_TEST_ALLOC_CAP / SZ4_TEST_FAIL_RESERVE, read by sz4_create),
 * out[2] = out-of-memory retries at a smaller piece in the last sz4_compress_blocks_device or batch
 * compression call, out[3] = the smallest piece size in bytes that call cut a pipeline run for. */
int sz4_debug_memory(sz4_ctx* ctx, uint64_t out[4]);

/* ---- decoder: the reference's smallz4cat ------------------------------------------------------
 * Decompress an LZ4 frame with the semantics of the reference decoder
 *   unlz4_userPtr(GET_BYTE, SEND_BYTES, dictionary, userPtr)      smallz4cat.c:112-360
 * over memory: modern and legacy frames, stored blocks, skipped block / content checksums,
 * content size and dictionary ID, an optional dictionary (its last 64 KiB precede the output),
 * a legacy frame ending after its first block shorter than 8 MiB.  Every byte is decoded on the
 * GPU (one wavefront per block).
 *   out_size  receives the decoded size, also when out_cap is too small (SZ4_E_CAPACITY):
 *             call with out = NULL, out_cap = 0 to query it
 * Returns SZ4_E_CORRUPT for a frame the reference decoder rejects (signature, version, truncated
 * frame, offset 0) or would misread (a length, literal run or offset crossing its block). */
int sz4_unlz4(sz4_ctx* ctx, const void* frame, uint64_t frame_len, const void* dict, uint64_t dict_len,
              void* out, uint64_t out_cap, uint64_t* out_size);

/* The same on device memory (frame, dictionary and output are device pointers) and a HIP stream;
 * returns after the stream has finished. */
int sz4_unlz4_device(sz4_ctx* ctx, const void* d_frame, uint64_t frame_len, const void* d_dict,
                     uint64_t dict_len, void* d_out, uint64_t out_cap, uint64_t* out_size, void* stream);

/* The reference decoder's callback types (smallz4cat.c:62-65). */
typedef unsigned char (*sz4_get_byte)(void* userPtr);
typedef void (*sz4_send_out)(const unsigned char* data, unsigned int numBytes, void* userPtr);

/* unlz4_userPtr(getByte, sendBytes, dictionary, userPtr) (smallz4cat.c:112-360) in bounded memory:
 * get_byte is called where the reference calls it on a valid frame (header, size words, payloads,
 * checksums; a legacy frame ends after its first block that decodes to less than 8 MiB); blocks are
 * decoded on the GPU a chunk at a time with the last 64 KiB of output as history, and send_bytes
 * receives the output in 64 KiB pieces followed by the remainder (the reference's flush points).
 * dict: the dictionary's bytes (its last 64 KiB are used) or NULL. */
int sz4_unlz4_stream(sz4_ctx* ctx, sz4_get_byte get_byte, sz4_send_out send_bytes, const void* dict, uint64_t dict_len,
                     void* user);

/* Device memory (bytes) the context holds: its scratch, staging and output buffers.  Buffers grow on
 * demand and are kept for the next call of the same kind. */
uint64_t sz4_device_bytes(sz4_ctx* ctx);

/* Release every device buffer and pinned host buffer the context holds (after its last call has
 * finished); the next call allocates again.  The context stays valid. */
void sz4_trim(sz4_ctx* ctx);

/* Bound the context's device memory to `bytes` (0 = no bound, the default).  A call that would grow
 * past it first releases the buffers it does not use itself -- those kept from calls of another kind:
 * the stream path's staging, dictionary tables, the decoder's output image -- and fails with
 * SZ4_E_NOMEM if that is not enough (the decoder then takes its block-by-block mode, which needs about
 * half the memory of its split mode, before it gives up).  The same release happens, bound or not, when
 * the device itself runs out of memory. */
void sz4_set_device_limit(sz4_ctx* ctx, uint64_t bytes);

/* Buffers the context has released under a device bound or device memory pressure (diagnostics). */
uint64_t sz4_released_buffers(sz4_ctx* ctx);

/* Pooled contexts (sz4_acquire) that hold more than `bytes` of device memory when they are released
 * are trimmed (sz4_trim) before they go back to the pool.  0 restores the default, 8 GiB. */
void sz4_set_pool_cap(uint64_t bytes);

/* Dictionary mode: the most match-finder rounds any chunk of the last stream call took (the
 * data-parallel finder assumes the same-letter shortcut intervals and reruns a chunk whose results imply
 * others; 1 = none to correct, 0 = no dictionary chunk, UINT32_MAX = a chunk fell back to the in-order
 * replay: after (largest block / 65 300) + 3 rounds -- one more interval settles per round --, or
 * SZ4_DICT_MAX_ROUNDS in the environment when the context was created). */
uint32_t sz4_dict_rounds(sz4_ctx* ctx);

/* Decoder diagnostics: the longest reference chain (hops to earlier sub-segments) the last split-mode decode
 * followed while packing its output (frames with blocks of >= 256 KiB payload), 0 when it decoded block by
 * block or no byte referred to another sub-segment. */
uint32_t sz4_unlz4_resolve_passes(sz4_ctx* ctx);
/* 1 when the last decode's block index came from the parallel index, 0 when the serial size-word walk
 * decided (a malformed frame, too many candidates, or SZ4_UNLZ4_INDEX=0). */
int sz4_unlz4_index_parallel(sz4_ctx* ctx);

/* Last error message of the context ("" if none). */
const char* sz4_last_error(sz4_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SMALLZ4_AMD_H */
