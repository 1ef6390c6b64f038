// sz4_internal.h -- descriptors shared by the host driver (sz4_host.cpp), its planner (sz4_plan.cpp) and the
// gfx950 kernels (sz4_kernels.hip, sz4_dict.hip), and the launchers between them: the
// compressor's take one PipeArgs (DictArgs in dictionary mode).  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace sz4 {

// constants of the reference format (smallz4.h:92-131)
constexpr int kMinMatch = 4;             // MinMatch
constexpr int kTailNoMatch = 12;         // BlockEndNoMatch
constexpr int kTailLiterals = 5;         // BlockEndLiterals
constexpr uint32_t kWindow = 65535;      // MaxDistance
constexpr uint32_t kSameLetter = 19 + 255 * 256;  // MaxSameLetter
constexpr int kGreedyMax = 3;            // ShortChainsGreedy
constexpr int kLazyMax = 6;              // ShortChainsLazy
constexpr uint32_t kHashMul = 48271;     // getHash32 multiplier
constexpr int kHashBits = 20;
constexpr uint64_t kNone = ~0ull;
// the parse's per-block flags (longFlag), set by every match finder (sz4_kernels.hip, sz4_dict.hip)
constexpr uint32_t kRmqLen = 274;  // match lengths from here on use the parse's range minima
constexpr uint32_t kFlagRmq = 1;   // the block has matches of kRmqLen+ (other than same-letter runs)
constexpr uint32_t kFlagRun = 2;   // a distance-1 match longer than MaxSameLetter (bounded chains)
constexpr int kStages = 6;  // runs, sort, find (sorted pass), find (long pass), parse, assemble

// device status word bits (one int per pipeline run)
constexpr int kStPrepRound = 2;   // k_lazy_correct corrected a shortcut interval: run sort/find/walk again
constexpr int kStInvariant = 4;   // a capacity invariant of the walk/token kernels failed: the frame is invalid

// one LZ4 block (all positions absolute byte offsets in the staged input)
struct Block {
  uint64_t start, end;     // [start, end)
  uint64_t low;            // lowest position a match may reference (reference dataZero)
  uint64_t cut;            // start-12 when the block re-inserts the previous tail (lookback), else kNone
  uint64_t tokOff;         // first 16-byte entry of this block in the Token area ((end-start)/2 + 4 of them)
  uint32_t prev;           // index of the previous block of the same stream, or kNoBlock
  uint32_t flags;          // kBlk* below
  uint32_t dpFirst;        // first DpSeg of this block (top segment first)
  uint32_t dpCount;        // number of DpSegs (0 when the block is too short to parse)
  uint32_t walkFirst;      // first token-walk sub-segment of this block
  uint32_t walkCount;      // number of token-walk sub-segments (ceil(n / kWalkSeg))
  uint32_t dpSize;         // positions per parse segment (dp_segment_size(n))
  uint32_t pad;
};
constexpr uint32_t kNoBlock = 0xFFFFFFFFu;
constexpr uint32_t kBlkLegacy = 1;         // always emitted compressed (legacy frame)

// targets [s0, s1) of one block, searched against the window [w0, s1)
struct Segment {
  uint64_t w0, s0, s1;
  uint64_t elemOff;        // offset (elements) of this segment's sort scratch
  uint64_t rankOff;        // offset (u32) of this segment's rank array (s1 - s0 entries)
  uint32_t block;
  uint32_t pad;
};

// positions [lo, hi) are skipped by the reference's same-letter shortcut
// (smallz4.h:631-643): not inserted into the chains and given (dist 1, La - (p - a))
struct Interval {
  uint64_t lo, hi;
  uint64_t a;              // the position whose distance-1 match starts the shortcut
  uint64_t La;             // its match length
};
// block b owns iv[b * kMaxIv .. b * kMaxIv + ivCount[b]); slot nblocks holds the final intervals of the
// previous chunk's last block when a stream is compressed in chunks (the first block's B.prev)
constexpr uint32_t kMaxIv = 136;  // > 8 MiB / 65300

// the optimal parse of one block runs as independent segments of B.dpSize positions (top segment
// first, k = 0): every segment is parsed at once from a guessed boundary, then k_dp_fix walks the
// boundaries top-down and re-parses each segment until it agrees with the speculative parse.
struct DpSeg {
  uint32_t block;
  uint32_t k;              // 0 = the segment holding the block's last parsed position
  uint32_t lo, hi;         // block-relative positions [lo, hi], parsed from hi down
};
// short segments give more parallelism; the serial part of the repair (k_dp_fix<false>) walks a
// block's boundaries one after the other, so large blocks keep longer segments
inline uint32_t dp_segment_size(uint64_t n) { return n <= 65536 ? 4096u : 8192u; }
constexpr uint32_t kMaxDpSegs = 2048;  // 8 MiB legacy block / 4096 (SZ4_DP_SIZE)

// the token walk runs as sub-segments of kWalkSeg positions, each walked speculatively from its
// first position and repaired by k_walk_fix; a sub-segment's matches live in 2 * walk_cap(r) slots of one
// 8-byte match record each (sz4_match_rec.h; speculative ones from walk_cap(r) on, repaired ones prepended
// below them), r being the sub-segment's positions
constexpr uint32_t kWalkSeg = 4096;
constexpr uint32_t kWalkCap = kWalkSeg / 4 + 2;
// matches of at least kMinMatch positions that start inside r positions, and two to spare: kWalkCap for a
// full sub-segment, less for a block's last one
constexpr uint32_t walk_cap(uint32_t r) { return r / 4 + 2 < kWalkCap ? r / 4 + 2 : kWalkCap; }
// The slots lie in the plan's Token area (Plan::WorkOffsets::tok: 16 bytes for each of a block's
// token_capacity(n) = n / 2 + 4 entries from Block::tokOff on, which is two records each): sub-segment k of a
// block has the records from 2 * tokOff + k * kWalkSeg on.  A full sub-segment uses 2 * kWalkCap of its
// kWalkSeg; the last one, of r positions, 2 * walk_cap(r) <= r / 2 + 4 of the r + 7 or more that remain.
constexpr uint64_t walk_slot_first(uint64_t tokOff, uint32_t k) { return 2 * tokOff + (uint64_t)k * kWalkSeg; }

// Sizes the planner (sz4_plan.cpp) shares with the kernels of sz4_kernels.hip that they are built for.
// The finders' LDS-window kernels hold a 64 KiB block and 16 bytes more:
constexpr uint32_t kFindLds = 65536 + 16;
constexpr uint32_t find_lds_bytes() { return kFindLds; }
// k_dp_fix<true> saves the speculative values it overwrites: kDpSide positions at most (or it gives up), and
// after them the range-minimum UP/DOWN keys down to the bottom of its convergence point's rmq block
// (kDpSide + 255 positions at most)
constexpr uint32_t kDpSide = 512;
constexpr uint32_t kDpSideKeys = kDpSide + 256;
constexpr uint32_t kDpSideStride = kDpSide + kDpSideKeys;
constexpr uint32_t dp_side_positions() { return kDpSideStride; }
// greedy/lazy replay: searched positions per walk sub-segment (<= 2 per 6 linked + 2), speculative and repaired
constexpr uint32_t kLazyCap = 1400;
constexpr uint32_t lazy_slots_per_walk() { return 2 * kLazyCap; }

// The buffers of one pipeline run, as every compressor launcher takes them: the host driver fills one
// PipeArgs per run (Pipe::args in sz4_host.cpp) once all of the run's buffers are reserved.  Arrays "per
// position" are indexed by the absolute staged position, like Block's fields.
struct PipeArgs {
  const uint8_t* in;        // the staged input (padded: the kernels read 4-byte windows past the last block)
  const Block* blocks;      // the plan's blocks
  uint32_t nblocks;
  const Segment* segs;      // the match search's segments
  uint32_t nsegs;
  const DpSeg* dpSegs;      // the parse's segments
  uint32_t ndp;
  uint32_t maxDpCount;      // the largest dpCount of the run's blocks (sizes k_dp_fix<false>'s LDS tables)
  const uint2* walkSegs;    // the token walk's sub-segments (block, index in the block)
  uint32_t nwalk;
  uint32_t maxChain;        // the reference's maxChainLength (<= kGreedyMax greedy, <= kLazyMax lazy, else optimal)
  Interval* iv;             // the same-letter shortcut intervals, kMaxIv per block (+ the ghost slot nblocks)
  uint32_t* ivCount;        // ... and how many each block has
  uint32_t* mlen;           // per position: the match length found (0: none)
  uint16_t* mdist;          // per position: its distance
  uint32_t* sel;            // per position: the parse's choice (k_prep writes the block tails)
  // cost / reach, per position, belong to the parse; before it they are pass 2's specLen / specDist
  // (k_find_big's left-maximal results, then the speculative carries of pass-2 piece heads), and after it
  // reach is the token walk's posList (each block's concatenated match positions and per-sub-segment records)
  uint32_t* cost;
  uint32_t* reach;
  uint32_t* longFlag;       // per block: kFlagRmq / kFlagRun, set by the match finders
  uint32_t* longBits;       // one bit per position marked for pass 2 (searched, not a shortcut interval)
  uint32_t* segLong;        // per segment: any such target
  uint64_t* segTail;        // per segment: k_find_big's state after its last target
  uint32_t* rank;           // per target: its rank in the segment's sort (written by pass 1)
  // the two halves of the sort elements: pass 1 sorts in elemA and leaves the sorted slot arrays in elemB;
  // elemA's per-slot words are free after the sort (the skip pointers of k_find_long9)
  uint2* elemA;
  uint2* elemB;
  uint32_t* rmqUp;          // the parse's range minima, (staged + nblocks + 8) words each
  uint32_t* rmqDown;
  uint2* dpSide;            // k_dp_fix<true>'s saved speculative values: dp_side_positions() per DpSeg
  uint4* dpRec;             // ... and one record per DpSeg
  uint4* segState;          // per DpSeg: the speculative parse's boundary state
  uint32_t* lazySlots;      // greedy/lazy replay: lazy_slots_per_walk() words per walk sub-segment
  uint64_t* walkSlots;      // token walk: the match records (walk_slot_first), in the plan's Token area
  uint4* walkState;         // per walk sub-segment: the state of the replay, then of the token walk
  uint32_t* ntok;          // per block: its token count
  uint32_t* blockBytes;     // per block: its size word; until the token walk, the lazy check's first difference
  uint64_t* offsets;        // per block: its offset in the frame body (slot nblocks: the body's size)
  int* status;              // the device status word (kSt*)
  bool ldsWindow;           // every segment's window fits the finders' LDS: the _lds kernels take the launch
  // launch_emit alone:
  uint8_t* out;             // the frame
  uint64_t headerLen;       // bytes the host writes in front of the first block
  const uint32_t* chosen;   // the lengths the token walk follows: sel (optimal levels) or mlen (greedy/lazy)
};
void launch_runs(const PipeArgs& a, hipStream_t s);
// pass 1 = k_find_sorted (each segment sorted first inside it, rank written), pass 2 = k_find_big /
// k_find_long9 / k_find (long matches and shortcut intervals)
void launch_find(int pass, const PipeArgs& a, hipStream_t s);
// dictionary mode (sz4_dict.hip and the in-order replay k_dict_matches), modern and legacy frames.
// dictBack = first insertion offset before the first block; last: 2^20 u32, prevH / prevX: 65536 u16
// each -- the reference's tables, kept in HBM between the chunks of one stream.  cont: the first block
// continues the stream of the previous launch, whose staged positions were `shift` (a multiple of 65536)
// higher; low0 = its dataZero.  hBlocks is the host copy of the plan; ph / pe: one u16 per staged
// position; keysA / keysB: dict_sort_keys_max() u64 each; temp: dict_sort_temp_bytes(); scBits:
// dict_sc_bits_bytes().  iv / ivCount: the assumed same-letter shortcut intervals per block; the parallel
// launch replaces them with the ones its results imply and raises kStPrepRound in *status when they
// differ (then the chunk is run again from its saved tables)
constexpr uint64_t kBlockMaxDict = 4ull << 20;     // MaxBlockSize (smallz4.h:124)
constexpr uint64_t kBlockMaxLegacy = 8ull << 20;   // MaxBlockSizeLegacy (smallz4.h:125)
struct DictArgs : PipeArgs {
  const Block* hBlocks;
  uint32_t dictBack, cont, shift, low0;
  int legacy;
  uint32_t* last;
  uint16_t *prevH, *prevX, *ph, *pe;
  uint64_t *keysA, *keysB;
  void* temp;
  uint64_t tempBytes;
  uint32_t* lzMasks;  // greedy/lazy levels: dict_lz_mask_bytes_per_walk() bytes per walk sub-segment (with walkState)
  uint64_t* scBits;
  uint2* runTab;      // runs covering whole 64-byte chunks: dict_run_table_bytes(staged) with runFlag
  uint32_t* runFlag;
  bool buildRuns;     // the first round of a chunk builds the table (the input does not change)
  bool guess;         // ... and appends its guess of the shortcut intervals to iv / ivCount (zeroed before)
};
// one wavefront replays the reference's match loop in order
void launch_dict(const DictArgs& a, hipStream_t s);
uint64_t dict_sort_keys_max();
uint64_t dict_sort_temp_bytes();  // rocPRIM's scratch for dict_sort_keys_max() keys; 0 if the query failed
uint64_t dict_sc_bits_bytes(uint32_t nb, uint64_t maxBlock);
uint64_t dict_run_table_bytes(uint64_t staged);
int launch_dict_parallel(const DictArgs& a, hipStream_t s);
uint64_t dict_lz_mask_bytes_per_walk();
// k_prep: the tail positions the reference never searches (lengths 0, literal choices)
void launch_prep(const PipeArgs& a, hipStream_t s);
// greedy/lazy levels: the parallel replay of the reference's skip bookkeeping (k_lazy_walk / k_lazy_fix /
// k_lazy_clear) over the assumed same-letter shortcut intervals, then their check (k_lazy_check /
// k_lazy_correct: status kStPrepRound = an interval list was corrected, run sort/find/walk again)
void launch_lazy(const PipeArgs& a, hipStream_t s);
void launch_parse(const PipeArgs& a, hipStream_t s);
// the token walk over a.chosen, the tokens, the block sizes and the frame body at a.out + a.headerLen
void launch_emit(const PipeArgs& a, hipStream_t s);

// decoder (sz4_unlz4.hip): one block of an LZ4 frame
struct UnBlock {
  uint64_t src;       // payload offset in the frame (decode queue: its address, the frame base being null)
  uint64_t dst;       // output offset (set by the host after the sizes pass; decode queue: the address)
  uint64_t size;      // decoded bytes (k_unlz4_sizes / k_unlz4_fix), kNone when malformed
  uint32_t len;       // payload bytes
  uint32_t stored;    // 1: uncompressed block
  uint32_t nseq;      // sequences recorded by k_unlz4_sizes
  uint32_t subFirst;  // split mode: first sub-segment of the block
  uint32_t subCount;  // split mode: its sub-segments (ceil(len / kUnSub))
  uint32_t pad;       // decode queue: the item's element width (read by the kTyped decoders alone)
};
// Split mode (frames with large blocks): every block is cut into sub-segments of kUnSub payload bytes,
// parsed speculatively from their first byte (k_unlz4_spec), joined to the true token chain per block
// (k_unlz4_fix), decoded into a u32 value-or-reference image one wavefront per sub-segment
// (k_unlz4_sub); k_unlz4_pack then follows every reference to an earlier sub-segment down to its byte
// while it packs the output, and reports the longest reference chain (hops) it followed.
constexpr uint32_t kUnSub = 8192;
constexpr uint32_t kUnSubCap = kUnSub / 3 + 4;    // sequences one walk over a sub-segment records
constexpr uint32_t kUnSplitMin = 256u << 10;      // a block of at least this many payload bytes: split mode
constexpr uint32_t kUnRef = 0x80000000u;          // image word: "same byte as output position (w & ~kUnRef)"
struct UnSub {
  uint32_t block, k;        // plan: block index, sub-segment index in the block
  uint32_t specN, specExit;  // k_unlz4_spec: sequences recorded, block-relative frame offset where it stopped
  uint32_t specFlags;        // 1: the walk met a malformed sequence at specExit, 2: it reached the block end
  uint32_t preN, specFrom;   // k_unlz4_fix: sequences re-parsed from the true entry, first speculative one kept
  uint32_t outRel, outLen;   // k_unlz4_fix: block-relative output offset and decoded bytes
  uint32_t specBytes;        // k_unlz4_spec: bytes its speculative list decodes
  // k_unlz4_join: the join computed from an ASSUMED entry (the previous sub-segment's speculative exit):
  // that entry, the exit it leads to, and 1: the previous walk was assumed to end there / 2: the join met a
  // malformed sequence / 4: this sub-segment reaches the block end.  k_unlz4_fix keeps it where the
  // assumption was the true chain's, and joins the others again from their true entry
  uint32_t joinEntry, joinExit, joinFlags;
};
// per sub-segment, k_unlz4_spec's side tables (u32 words): the token-start mask (kUnSub / 32 words), the
// mask's prefix bit counts per word (u16, kUnSub / 64 words), and each speculative sequence's output offset
// from the sub-segment's first token (kUnSubCap words) -- k_unlz4_fix's rank and byte count in O(1)
constexpr uint32_t kUnAuxWords = (kUnSub / 32 + kUnSub / 64 + kUnSubCap + 63) / 64 * 64;
void launch_unlz4_index(const uint8_t* f, uint64_t n, UnBlock* blk, uint64_t maxBlocks, uint64_t* meta, hipStream_t s);
// the same result from the parallel index (candidate offsets, then one wavefront over their successors;
// falls back to the serial walk in the same launch when the candidates cannot settle the chain)
void launch_unlz4_index_par(const uint8_t* f, uint64_t n, void* scratch, UnBlock* blk, uint64_t maxBlocks, uint64_t* meta,
                            hipStream_t s);
uint64_t unlz4_ix_scratch_bytes(uint64_t n);
uint64_t unlz4_ix_cap(uint64_t n);
// sequence list: unlz4_seq_entries(frame length, blocks) uint4 entries (block bi's at src / 3 + 2 bi)
uint64_t unlz4_seq_entries(uint64_t frameLen, uint32_t nb);
void launch_unlz4_sizes(const uint8_t* f, uint64_t n, UnBlock* blk, uint32_t nb, uint4* seq, hipStream_t s);
// flags: nb done flags, then the status word, then the ticket (zeroed before the launch)
void launch_unlz4_blocks(const uint8_t* f, uint64_t n, const UnBlock* blk, uint32_t nb, const uint4* seq, uint8_t* out,
                         const uint8_t* dict, uint64_t dl, uint32_t* flags, hipStream_t s);
// independent mode (the batch decoder): every block decodes on its own -- a match source below the block's
// first output byte reads 0 (the reference's zero-initialised history), never another block's output, and no
// block waits for another.  flags: the status word alone (zeroed before the launch)
void launch_unlz4_blocks_indep(const uint8_t* f, uint64_t n, const UnBlock* blk, uint32_t nb, const uint4* seq,
                               uint8_t* out, uint32_t* flags, hipStream_t s);
// batch decoder plan: block b is the bare LZ4 block f[ext[2b], ext[2b + 1]) (4-byte size word + payload, at
// least 4 bytes); fills src / len / stored and sets *status when a size word disagrees with its extent
void launch_unlz4_batch_plan(const uint8_t* f, const uint64_t* ext, uint32_t nb, UnBlock* blk, uint32_t* status,
                             hipStream_t s);
// decode queue (sz4_dq_enqueue): the caller's device tables, `count` entries each, read and written by the
// kernels alone.  Item i is the bare block [src[i], src[i] + srcSizes[i]) and decodes to dst[i] (capacity
// dstCaps[i]) as an item of width elems[i] (null: 1); outSizes and status (kItem*, SZ4_ITEM_*) are the result
constexpr uint32_t kMaxFrameBlock = (uint32_t)(kBlockMaxLegacy + kBlockMaxLegacy / 255 + 16);  // LZ4 compress bound
constexpr uint32_t kItemOk = 0, kItemCorrupt = 1, kItemCapacity = 2, kItemArg = 3, kItemQueue = 4, kItemInternal = 5;
struct DqTables {
  const uint64_t* src;
  const uint32_t* srcSizes;
  const uint64_t* dst;
  const uint32_t* dstCaps;
  const uint8_t* elems;
  uint32_t* outSizes;
  uint32_t* status;
};
// plan (one workgroup: checks, running source bytes against maxSrc, the scan of the sequence-list needs into
// seqOff), size pass and decode pass, one wavefront per item: three kernels in a row on s, nothing else.
// blk, seqOff: count entries; seq: unlz4_seq_entries(maxSrc, count) entries.  count > 0
void launch_unlz4_dq(const DqTables& T, uint32_t count, uint64_t maxSrc, UnBlock* blk, uint64_t* seqOff, uint4* seq,
                     hipStream_t s);
// split mode: seq holds 2 * kUnSubCap entries per sub-segment (re-parsed prefix, speculative list), masks
// kUnAuxWords words per sub-segment (the token-start mask and k_unlz4_spec's side tables)
void launch_unlz4_split_sizes(const uint8_t* f, uint64_t n, UnBlock* blk, uint32_t nb, UnSub* subs, uint32_t nsub,
                              uint4* seq, uint32_t* masks, hipStream_t s);
// image: one u32 per output byte; hops: one u32 (zeroed before k_unlz4_pack: the longest reference chain it followed)
void launch_unlz4_split_decode(const uint8_t* f, uint64_t n, const UnBlock* blk, const UnSub* subs, uint32_t nsub,
                               const uint4* seq, uint32_t* image, const uint8_t* dict, uint64_t dl, hipStream_t s);
void launch_unlz4_pack(uint32_t* image, uint64_t total, uint8_t* out, uint32_t* hops, hipStream_t s);

// ragged batch API (sz4_batch.hip).  One item of a pipeline run: `size` bytes at device address `src` (any
// alignment) are staged at [start, start + size); starts are multiples of kBatchAlign and ascending
constexpr uint64_t kBatchAlign = 64;
struct BatchItem {
  uint64_t src, start, size;
};
// stages the items and zero-fills every other byte of staged[0, stagedBytes) (the gaps between items and the
// pad after the last one); stagedBytes is a multiple of 16 and `staged` 16-byte aligned
void launch_batch_gather(const BatchItem* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s);
// typed items (sz4_compress_batch_typed_device / sz4_unlz4_batch_typed_device): an item of element width
// `elem` (1, 2, 4 or 8).  For the gather src is a device address and start the staged offset, as in BatchItem;
// for the merge src is the item's offset in the decoder's scratch and start its offset in the caller's buffer
struct BatchTyped {
  uint64_t src, start;
  uint32_t size, elem;
};
// launch_batch_gather with the byte-plane split of every item of width > 1 folded in (the staged item is
// split(item, elem): byte k of every whole element together, plane after plane, then the tail bytes)
void launch_batch_gather_planes(const BatchTyped* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s);
// the inverse: to[start, start + size) = merge(from[src, src + size), elem) for every item; the items are
// non-empty, ascending and back to back in `to` (starts are running sums from 0 to `total`); `to` has any alignment
void launch_batch_merge(const BatchTyped* items, uint32_t n, const uint8_t* from, uint8_t* to, uint64_t total, hipStream_t s);
// filtered items (sz4_compress_batch_filtered_device / sz4_unlz4_batch_filtered_device): a table with an item
// of SZ4_FILTER_BITS holds (filter << kBatchFilterShift) | width in `elem` and goes to these two, which shuffle
// such an item into its bit planes (and back) and treat every other item as the two above do
constexpr uint32_t kBatchFilterShift = 8;
void launch_batch_gather_bits(const BatchTyped* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s);
void launch_batch_merge_bits(const BatchTyped* items, uint32_t n, const uint8_t* from, uint8_t* to, uint64_t total, hipStream_t s);
// moves compressed blocks to their caller-order place: entry k copies len bytes from `from + src` to `to + dst`
// (the host cuts long blocks into entries of at most kBatchMoveMax bytes, so the work is balanced by bytes)
constexpr uint64_t kBatchMoveMax = 65536;
struct BatchMove {
  uint64_t src, dst, len;
};
void launch_batch_move(const BatchMove* moves, uint32_t n, const uint8_t* from, uint8_t* to, hipStream_t s);

// compress queue (sz4_cq_enqueue): the caller's device tables, `count` entries each, around one ragged run whose
// blocks are the non-empty items in caller order.  map[i] is the block of the first non-empty item at or after
// item i (nblocks: there is none), with kCqEmpty set when item i itself is empty
constexpr uint32_t kCqEmpty = 0x80000000u;
struct CqTables {
  const uint64_t* src;   // the items' device addresses (an empty item's entry is not read)
  const uint32_t* map;   // null in a sized queue: item i is block i
  uint32_t count;
  uint8_t* out;          // where the run writes its blocks
  uint64_t* blockPtrs;   // results: every block's address in `out`, its bytes (size word included), kItem*
  uint32_t* blockSizes;
  uint32_t* status;
  uint64_t* total;       // the bytes written to `out` (may be null)
};
// before the gather: the sources into the run's resident item table (BatchTyped when `typed`, else BatchItem;
// start and elem stay as uploaded), and every item's first status.  A null source of a non-empty item gets
// size 0 in the table -- the gather stages zeros for it, nothing is read -- and kItemArg.  Also clears P's
// status word, longFlag, ghost interval count and (no blocks) body size, which a synchronous run memsets
void launch_cq_items(const CqTables& T, const PipeArgs& P, void* items, bool typed, hipStream_t s);
// a sized queue's launch_cq_items (sz4_cq_enqueue_sized; T.map is null, P.nblocks == T.count): srcSizes is the
// caller's DEVICE table of this enqueue's sizes, `slots` the queue's resident Slot table (sz4_slot_plan.h).
// Besides launch_cq_items' work it rewrites P.blocks, P.segs and P.dpSegs for those sizes, and decides
// kItemCapacity for a size above its slot's capacity
struct Slot;
void launch_cq_plan(const CqTables& T, const uint32_t* srcSizes, const Slot* slots, const PipeArgs& P, void* items, bool typed,
                    hipStream_t s);
// zeroes [p, p + bytes rounded up to 16) with a kernel (p is 16-byte aligned)
void launch_cq_zero(void* p, uint64_t bytes, hipStream_t s);
// after the assembly: addresses and sizes from P.offsets / P.blockBytes; kItemInternal for every item, with
// size 0 and a total of 0, when P's status word carries kStInvariant
void launch_cq_finish(const CqTables& T, const PipeArgs& P, hipStream_t s);

}  // namespace sz4
