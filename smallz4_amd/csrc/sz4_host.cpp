// sz4_host.cpp -- host driver behind the C ABI in include/smallz4_amd.h.
//
// Plans a job (sz4_plan.h: one Plan per context, rebuilt when its key differs),
// keeps device scratch resident in HBM (sz4_mem.h: grow-only, so repeated calls
// allocate nothing), launches the kernel pipeline of sz4_kernels.hip on one HIP
// stream and assembles the frame.
//
// Three job shapes:
//   * independent blocks (sz4_compress_blocks_device): every block compressed
//     as the reference compresses a stand-alone input -- the data-parallel
//     shape that fills the GPU (BASELINE configs 1-4);
//   * ragged batches (sz4_compress_batch_device): the same, over many separate
//     device buffers of different sizes, one block each;
//   * one reference stream (sz4_lz4): the exact block structure of
//     smallz4::compress (smallz4.h:476-813): 4 MiB blocks that see the previous
//     64 KiB, or 8 MiB independent legacy blocks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <string>
#include <new>
#include <vector>

#include "../../include/smallz4_amd.h"
#include "sz4_internal.h"
#include "sz4_mem.h"
#include "sz4_plan.h"

using namespace sz4;

namespace {

constexpr uint64_t kPad = 64;                 // bytes of slack after every staged input
// batch API pieces: at most 448 MiB of input, split evenly (a rank's 1.25 GiB slice of configs[4]: three
// pieces of 427 MiB), so that the scratch (48.6 B per piece byte at 256 KiB blocks) stays under ~21 GiB.
// Round 5's 1.5 GiB pieces took ~61 GiB for +14 % on configs[4]: the slice in ONE piece runs the per-block
// parse repair wavefronts of its 5120 blocks together, one latency-bound launch instead of one per piece
constexpr uint64_t kBatchChunkDefault = 448ull << 20;
constexpr uint64_t kScratchPerByte = 50;     // device scratch per piece byte, upper bound (36-49 measured)
constexpr uint64_t kPieceFloor = 16ull << 20;  // smallest batch piece the out-of-memory retry goes down to
constexpr uint64_t kBlockMax = kBlockMaxDict;  // MaxBlockSize (smallz4.h:124)
// dictionary rounds before the in-order replay takes the chunk: each round confirms a longer prefix of every
// block; a wrongly assumed interval may take two rounds (dropped in one, its real start inserted in the
// next: ADVICE r05), so a chunk needs at most 2 x (intervals per block) + 1 rounds, and a block holds at
// most one interval per MaxSameLetter + 1 bytes; a chunk that needs more than that (the old
// cap was 4 x kMaxIv = 544 rounds) goes to the replay
uint32_t dict_round_cap(uint64_t maxBlock) { return 2u * (uint32_t)(maxBlock / (kSameLetter + 1)) + 3u; }
// smallz4's frame header (smallz4.h:478-496: magic, version 1 with independent-block flag clear, 4 MiB blocks,
// header checksum) and the legacy frame's magic
constexpr uint8_t kFrameHeader[7] = {0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF};
constexpr uint8_t kLegacyMagic[4] = {0x02, 0x21, 0x4C, 0x18};

uint32_t xxh32_small(const uint8_t* d, size_t n)
{
  const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P5 = 374761393u;
  uint32_t h = P5 + (uint32_t)n;
  for (size_t i = 0; i < n; i++) {
    h += d[i] * P5;
    h = ((h << 11) | (h >> 21)) * P1;
  }
  h ^= h >> 15;
  h *= P2;
  h ^= h >> 13;
  h *= P3;
  h ^= h >> 16;
  return h;
}

// Everything one pipeline run names on the device, and the plan it runs: the context holds one for its calls,
// a compress queue another (held) one, so that neither moves or overwrites what the other's kernels read.
// Every DevBuf is constructed on the owner's budget and enters its list there.
struct Pipe {
  DevBuf staged, blocks, segs, iv, ivCount, rank, mlen, mdist;
  DevBuf cost, ntok, blockBytes, offsets, status;
  DevBuf dpSegs, reach, segState, walkSegs, walkState;
  DevBuf longFlag, longBits, segLong, segTail;
  DevBuf dpRec;       // the parallel parse-boundary repair's records
  DevBuf work;        // the arrays whose lifetimes do not overlap, at plan.off (Plan::work_layout)
  DevBuf batchItems;  // ragged runs: the gather's item table
  // The block plan of the current run: one object for every kind of call, rebuilt when its key differs.
  // Its device copy (blocks, segments, parse segments, walk sub-segments) is fresh while it holds this
  // version of the plan at these four addresses: repeated calls on the same shape skip the uploads
  Plan plan;
  uint64_t uploadedVersion = ~0ull;
  const void* uploadedAt[4] = {};

  explicit Pipe(Budget& b, bool keep = false)
      : staged(b, keep), blocks(b, keep), segs(b, keep), iv(b, keep), ivCount(b, keep), rank(b, keep), mlen(b, keep),
        mdist(b, keep), cost(b, keep), ntok(b, keep), blockBytes(b, keep), offsets(b, keep), status(b, keep),
        dpSegs(b, keep), reach(b, keep), segState(b, keep), walkSegs(b, keep), walkState(b, keep), longFlag(b, keep),
        longBits(b, keep), segLong(b, keep), segTail(b, keep), dpRec(b, keep), work(b, keep), batchItems(b, keep) {}
  template <class T>
  T* work_at(uint64_t off) const { return reinterpret_cast<T*>(work.as<uint8_t>() + off); }
  uint32_t* sel() const { return work.as<uint32_t>(); }
  // the scratch of a run of the plan over `stagedBytes` of staged input (staging and the item table are the caller's)
  hipError_t reserve(uint64_t stagedBytes);
  // the launchers' view of the buffers for the plan.  A reserve can move a buffer, so this runs after every
  // reserve of the call (reserve; the dictionary's own reserves move only dict* buffers)
  PipeArgs args(uint32_t maxChain, const uint8_t* in, uint8_t* out, uint64_t hdrLen) const;
  // the plan's four tables to their buffers, on s
  hipError_t upload_plan(hipStream_t s) const;
  // a pipe that ends before its budget's owner does (a compress queue's)
  void detach()
  {
    for (DevBuf* b : {&staged, &blocks, &segs, &iv, &ivCount, &rank, &mlen, &mdist, &cost, &ntok, &blockBytes, &offsets,
                      &status, &dpSegs, &reach, &segState, &walkSegs, &walkState, &longFlag, &longBits, &segLong, &segTail,
                      &dpRec, &work, &batchItems})
      b->detach();
  }
};

hipError_t Pipe::reserve(uint64_t stagedBytes)
{
  const uint64_t nb = plan.blocks.size();
  hipError_t e = hipSuccess;
  (e = blocks.reserve(nb * sizeof(Block) + 64)) ||
      (e = segs.reserve(plan.segs.size() * sizeof(Segment) + 64)) ||
      (e = iv.reserve((nb + 1) * kMaxIv * sizeof(Interval) + 64)) ||
      (e = ivCount.reserve((nb + 1) * 4 + 64)) ||
      (e = rank.reserve(plan.rankTotal * 4 + 64)) ||
      (e = mlen.reserve(stagedBytes * 4 + 64)) ||
      (e = mdist.reserve(stagedBytes * 2 + 64)) ||
      (e = cost.reserve((stagedBytes + nb + 8) * 4)) ||
      (e = ntok.reserve(nb * 4 + 64)) ||
      (e = blockBytes.reserve(nb * 4 + 64)) ||
      (e = offsets.reserve((nb + 1) * 8 + 64)) ||
      (e = status.reserve(64)) ||
      (e = dpSegs.reserve(plan.dp.size() * sizeof(DpSeg) + 64)) ||
      // (after the parse the token walk's records live here: a uint4 per walk sub-segment and a uint2 per block,
      // which outgrow the positions only where blocks stage nothing -- a sized queue's slots of capacity 0)
      (e = reach.reserve(std::max<uint64_t>(stagedBytes * 4, plan.walk.size() * sizeof(uint4) + nb * sizeof(uint2)) + 64)) ||
      (e = segState.reserve(plan.dp.size() * sizeof(uint4) + 64)) ||
      (e = dpRec.reserve(plan.dp.size() * sizeof(uint4) + 64)) ||
      (e = walkSegs.reserve(plan.walk.size() * sizeof(uint2) + 64)) ||
      (e = walkState.reserve(plan.walk.size() * sizeof(uint4) + 64)) ||
      (e = longFlag.reserve(nb * 4 + 64)) ||
      (e = longBits.reserve(stagedBytes / 8 + 64)) ||
      (e = segLong.reserve(plan.segs.size() * 4 + 64)) ||
      (e = segTail.reserve(plan.segs.size() * 8 + 64)) ||
      (e = work.reserve(plan.work_layout(stagedBytes)));
  return e;
}

PipeArgs Pipe::args(uint32_t maxChain, const uint8_t* in, uint8_t* out, uint64_t hdrLen) const
{
  PipeArgs a{};
  a.in = in;
  a.blocks = blocks.as<Block>();
  a.nblocks = (uint32_t)plan.blocks.size();
  a.segs = segs.as<Segment>();
  a.nsegs = (uint32_t)plan.segs.size();
  a.dpSegs = dpSegs.as<DpSeg>();
  a.ndp = (uint32_t)plan.dp.size();
  a.maxDpCount = plan.maxDpCount;
  a.walkSegs = walkSegs.as<uint2>();
  a.nwalk = (uint32_t)plan.walk.size();
  a.maxChain = maxChain;
  a.iv = iv.as<Interval>();
  a.ivCount = ivCount.as<uint32_t>();
  a.mlen = mlen.as<uint32_t>();
  a.mdist = mdist.as<uint16_t>();
  a.sel = sel();
  a.cost = cost.as<uint32_t>();
  a.reach = reach.as<uint32_t>();
  a.longFlag = longFlag.as<uint32_t>();
  a.longBits = longBits.as<uint32_t>();
  a.segLong = segLong.as<uint32_t>();
  a.segTail = segTail.as<uint64_t>();
  a.rank = rank.as<uint32_t>();
  const Plan::WorkOffsets& off = plan.off;
  a.elemA = work.as<uint2>();
  a.elemB = work_at<uint2>(off.elemB);
  a.rmqUp = work_at<uint32_t>(off.rmqUp);
  a.rmqDown = work_at<uint32_t>(off.rmqDown);
  a.dpSide = work_at<uint2>(off.side);
  a.dpRec = dpRec.as<uint4>();
  a.segState = segState.as<uint4>();
  a.lazySlots = work_at<uint32_t>(off.lazy);
  a.walkSlots = work_at<uint64_t>(off.tok);
  a.walkState = walkState.as<uint4>();
  a.ntok = ntok.as<uint32_t>();
  a.blockBytes = blockBytes.as<uint32_t>();
  a.offsets = offsets.as<uint64_t>();
  a.status = status.as<int>();
  a.ldsWindow = plan.ldsWindow;
  a.out = out;
  a.headerLen = hdrLen;
  // optimal levels tokenize the parse's choices, greedy/lazy levels the (skip-filtered) matches
  a.chosen = maxChain > (uint32_t)kGreedyMax ? a.sel : a.mlen;
  return a;
}

hipError_t Pipe::upload_plan(hipStream_t s) const
{
  hipError_t e = hipSuccess;
  (e = hipMemcpyAsync(blocks.p, plan.blocks.data(), plan.blocks.size() * sizeof(Block), hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(segs.p, plan.segs.data(), plan.segs.size() * sizeof(Segment), hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(dpSegs.p, plan.dp.data(), plan.dp.size() * sizeof(DpSeg), hipMemcpyHostToDevice, s)) ||
      (e = hipMemcpyAsync(walkSegs.p, plan.walk.data(), plan.walk.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
  return e;
}

}  // namespace

struct sz4_ctx {
  int device = 0;
  std::string err;
  bool timing = false;
  hipEvent_t ev[kStages + 1] = {};
  float stageMs[kStages] = {};
  uint32_t lastBlocks = 0;
  int stopAfter = 0;
  uint32_t lastChain = 0;

  // Device scratch.  Every DevBuf is constructed on `budget` and enters its list there: accounting, the device
  // limit, shed(), sz4_trim and sz4_destroy see a buffer because it is declared, and nowhere else is it named.
  Budget budget;
  Pipe pipe{budget};  // the pipeline's buffers and the block plan of the current run
  DevBuf dictLast{budget}, dictPrevH{budget}, dictPrevX{budget};  // dictionary mode: the reference's hash table and both chains
  // dictionary mode on the whole GPU (sz4_dict.hip)
  DevBuf dictPH{budget}, dictPE{budget}, dictKeys{budget}, dictTemp{budget}, dictSc{budget}, dictSnap{budget}, dictRuns{budget};
  DevBuf dictLz{budget};
  uint32_t dictRounds = 0;  // most rounds a dictionary chunk of the last call took (~0u: one fell back to the in-order replay)
  uint32_t dictMaxRounds = getenv("SZ4_DICT_MAX_ROUNDS") && atoi(getenv("SZ4_DICT_MAX_ROUNDS")) > 0
                               ? (uint32_t)atoi(getenv("SZ4_DICT_MAX_ROUNDS")) : 0u;  // tests: force the replay (0: dict_round_cap)
  bool dictNoGuess = getenv("SZ4_DICT_NO_GUESS") != nullptr;  // A/B: the first round assumes no shortcut interval
  uint64_t dictTempBytes = 0;  // rocPRIM radix sort scratch for dictKeys (queried on first use)
  // stream path: two chunks' blocks (chunk i+1 computes while chunk i downloads) and two chunks' staged input
  // (chunk i+1 uploads while chunk i computes)
  DevBuf chunkOut[2]{DevBuf{budget}, DevBuf{budget}};
  DevBuf stagedS[2]{DevBuf{budget}, DevBuf{budget}};
  HostBuf hostIn[2], hostOut[2];
  uint64_t streamChunk = 64ull << 20;  // stream path: input bytes per chunk (rounded to whole blocks)
  uint64_t batchChunk = kBatchChunkDefault;  // sz4_compress_blocks_device: input bytes per internal pipeline run
  bool batchChunkSet = false;          // set explicitly (sz4_set_batch_chunk, SZ4_BATCH_CHUNK): no free-memory cap
  bool batchChunked = false;           // the last sz4_compress_blocks_device call ran in several pieces
  uint64_t pieceRetries = 0;           // sz4_debug_memory: the last blocks or batch call's out-of-memory retries
  uint64_t pieceMin = 0;               // ... and the smallest piece size (bytes) a pipeline run of it was cut for
  // stream path, chunk continuation: the previous chunk's last block's final shortcut intervals
  // (ghost slot nblocks of iv/ivCount, B.prev of the first block), uploaded by runs whose RunMode says so
  std::vector<Interval> ghostIv;
  uint32_t ghostN = 0;
  // decoder (sz4_unlz4*); split mode: sub-segments, their token-start masks, the u32 image
  DevBuf unBlk{budget}, unMeta{budget}, unFlags{budget}, unFrame{budget}, unDict{budget}, unOut{budget}, unSeq{budget};
  DevBuf unSubs{budget}, unMasks{budget}, unImage{budget};
  DevBuf unIx{budget};                    // decoder: the parallel frame index's candidates and successors
  // ragged batch API: the block mover's table and the staging area of a piece that runs as two pipeline
  // runs (sz4_compress_batch_device); the batch decoder's extent table
  DevBuf batchMoves{budget}, batchTmp{budget}, unBatch{budget};
  // typed batch decoder (sz4_unlz4_batch_typed_device): the decoded split items, and k_batch_merge's item table
  DevBuf unPlanes{budget}, mergeItems{budget};
  hipEvent_t evGather[2] = {};  // timing: around k_batch_gather / k_batch_gather_planes
  float gatherMs = 0;
  hipEvent_t evMerge[2] = {};   // timing: around k_batch_merge
  float mergeMs = 0;
  bool unIndexSerial = getenv("SZ4_UNLZ4_INDEX") && atoi(getenv("SZ4_UNLZ4_INDEX")) == 0;  // A/B: the one-lane walk
  std::vector<UnBlock> hUn;
  std::vector<UnSub> hSub;
  bool unSplit = false;  // the last planned frame decodes in split mode
  uint32_t unResolvePasses = 0;  // the longest reference chain the last split-mode decode's pack followed
  bool unIndexParallel = false;  // the last frame index came from the parallel index (not the serial walk)
  int unSplitMode = getenv("SZ4_UNLZ4_SPLIT") ? atoi(getenv("SZ4_UNLZ4_SPLIT")) : -1;  // -1 auto, 0 never, 1 always
  bool dictSerial = getenv("SZ4_DICT_SERIAL") != nullptr;  // A/B and tests: the in-order replay for every chunk

  std::vector<uint32_t> hostBytes;

  hipStream_t stream = nullptr;  // the stream path's compute stream
  hipStream_t upStream = nullptr, downStream = nullptr;  // its upload and download streams
  hipEvent_t evUp[2] = {}, evDone[2] = {};  // per staging slot: upload complete, chunk computed
  bool pooled = false;           // handed out by sz4_acquire
  std::mutex* poolMu = nullptr;
  std::vector<sz4_ctx*>* poolIdle = nullptr;

  // a new call: later reserves record it, and a growing call may release what earlier calls left
  void begin_call()
  {
    err.clear();
    budget.gen++;
  }

  int fail(int code, const char* what, hipError_t e = hipSuccess)
  {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    err = buf;
    return code;
  }

  // before a blocks or batch piece is tried again at a smaller size: the failed attempt is no error of the
  // call, and what it reserved goes back first -- the buffers it grew in order, up to the one that failed,
  // carry the current call's mark, so shed() would keep them and the smaller piece would have to fit beside
  // the larger one's.  Nothing runs on them: every earlier piece of the call has finished.  Afterwards the
  // retry finds what a fresh context would (queues keep their held scratch)
  void retry_smaller()
  {
    err.clear();
    for (DevBuf* b : budget.bufs)
      if (!b->held) b->release();
    pipe.uploadedVersion = ~0ull;
    pieceRetries++;
  }
};

namespace {

int reserve_all(sz4_ctx* c, uint64_t stagedBytes)
{
  if (hipError_t e = c->pipe.reserve(stagedBytes)) return c->fail(SZ4_E_NOMEM, "device allocation", e);
  return SZ4_OK;
}

void mark(sz4_ctx* c, int i, hipStream_t s)
{
  if (c->timing) hipEventRecord(c->ev[i], s);
}

// sz4_debug_stop_after: the run ends here, once what it has enqueued has finished
int stop_here(sz4_ctx* c, hipStream_t s)
{
  return hipStreamSynchronize(s) == hipSuccess ? SZ4_OK : c->fail(SZ4_E_DEVICE, "pipeline");
}

int pipeline_finish(sz4_ctx* c, const uint8_t* hdr, uint64_t hdrLen, bool endMark, uint8_t* out, uint64_t outCap,
                    uint64_t* outSize, hipStream_t s);

// What a pipeline run takes over from the stream it belongs to.  The default is a run of independent
// blocks: no dictionary, no ghost slot.
struct RunMode {
  int64_t dictBack = -1;  // >= 0: dictionary mode, first insertion this far before the first block
  int legacy = 0;         // dictionary mode: a legacy frame (every block starts from empty tables)
  uint32_t cont = 0, shift = 0, low0 = 0;  // dictionary mode: the previous chunk's table position (DictArgs)
  bool ghost = false;     // the first block's B.prev is the ghost slot: upload the context's ghostIv into it
};

// run the kernel pipeline over the planned blocks of the staged input `in`; frame goes to `out`.
// finish = false: return once every kernel is enqueued (pipeline_finish collects the result)
int run_pipeline(sz4_ctx* c, const RunMode& mode, uint32_t maxChain, const uint8_t* in, const uint8_t* hdr, uint64_t hdrLen,
                 bool endMark, uint8_t* out, uint64_t outCap, uint64_t* outSize, hipStream_t s, bool finish = true)
{
  const uint32_t nb = (uint32_t)c->pipe.plan.blocks.size();
  c->lastChain = maxChain;
  hipError_t e;
  const void* at[4] = {c->pipe.blocks.p, c->pipe.segs.p, c->pipe.dpSegs.p, c->pipe.walkSegs.p};
  const bool fresh = c->pipe.uploadedVersion == c->pipe.plan.version && memcmp(at, c->pipe.uploadedAt, sizeof at) == 0;
  if (!fresh && (e = c->pipe.upload_plan(s))) return c->fail(SZ4_E_DEVICE, "upload plan", e);
  c->pipe.uploadedVersion = c->pipe.plan.version;
  memcpy(c->pipe.uploadedAt, at, sizeof at);
  const PipeArgs P = c->pipe.args(maxChain, in, out, hdrLen);
  if ((e = hipMemsetAsync(P.status, 0, 4, s)) || (e = hipMemsetAsync(P.longFlag, 0, nb * 4, s)))
    return c->fail(SZ4_E_DEVICE, "upload plan", e);
  // ghost slot nb: the previous chunk's last block (only its intervals are read, through B.prev).  The
  // sources of these asynchronous copies live in the context: the stream path returns before they run
  c->ghostN = mode.ghost ? (uint32_t)c->ghostIv.size() : 0u;
  if ((c->ghostN && (e = hipMemcpyAsync(P.iv + (uint64_t)nb * kMaxIv, c->ghostIv.data(), c->ghostN * sizeof(Interval),
                                        hipMemcpyHostToDevice, s))) ||
      (e = hipMemcpyAsync(P.ivCount + nb, &c->ghostN, 4, hipMemcpyHostToDevice, s)))
    return c->fail(SZ4_E_DEVICE, "upload intervals", e);
  const bool dictMode = mode.dictBack >= 0;

  mark(c, 0, s);
  if (!dictMode) launch_runs(P, s);
  mark(c, 1, s);
  if (dictMode && maxChain > 0) {
    // dictionary mode (modern and legacy frames): the data-parallel match finder of sz4_dict.hip, in
    // rounds until its assumed same-letter shortcut intervals are the ones its results imply; then the
    // usual parse
    if ((e = c->dictLast.reserve(sizeof(uint32_t) << 20)) || (e = c->dictPrevH.reserve(2 * 65536)) ||
        (e = c->dictPrevX.reserve(2 * 65536)))
      return c->fail(SZ4_E_NOMEM, "dictionary tables", e);
    DictArgs A{P};
    A.hBlocks = c->pipe.plan.blocks.data();
    A.dictBack = (uint32_t)mode.dictBack;
    A.cont = mode.cont;
    A.shift = mode.shift;
    A.low0 = mode.low0;
    A.legacy = mode.legacy;
    A.last = c->dictLast.as<uint32_t>();
    A.prevH = c->dictPrevH.as<uint16_t>();
    A.prevX = c->dictPrevX.as<uint16_t>();
    if (c->dictSerial) {
      launch_dict(A, s);  // A/B and tests: the reference's loop replayed in order by one wavefront
    } else {
      const uint64_t staged = c->pipe.plan.blocks.back().end + 64;
      uint64_t maxBlock = 0;
      for (const Block& B : c->pipe.plan.blocks) maxBlock = std::max<uint64_t>(maxBlock, B.end - B.start);
      // rocPRIM's scratch size, queried once per context on its own device (0: the query failed)
      if (!c->dictTempBytes && !(c->dictTempBytes = dict_sort_temp_bytes()))
        return c->fail(SZ4_E_DEVICE, "dictionary sort: scratch size query");
      const uint64_t lastBytes = sizeof(uint32_t) << kHashBits, slotBytes = 2 * 65536;
      if ((e = c->dictPH.reserve(staged * 2)) || (e = c->dictPE.reserve(staged * 2)) ||
          (e = c->dictKeys.reserve(2 * dict_sort_keys_max() * 8)) || (e = c->dictTemp.reserve(c->dictTempBytes + 64)) ||
          (e = c->dictSc.reserve(dict_sc_bits_bytes(nb, maxBlock))) ||
          (e = c->dictSnap.reserve(lastBytes + 2 * slotBytes)) || (e = c->dictRuns.reserve(dict_run_table_bytes(staged))) ||
          (e = c->dictLz.reserve(c->pipe.plan.walk.size() * dict_lz_mask_bytes_per_walk() + 64)))
        return c->fail(SZ4_E_NOMEM, "dictionary scratch", e);
      // the carried tables as this chunk found them: a round that finds other shortcut intervals starts
      // again from here (legacy frames carry nothing: every block starts from empty tables)
      uint8_t* snap = c->dictSnap.as<uint8_t>();
      auto tables = [&](bool save) -> hipError_t {
        hipError_t r;
        uint8_t* t[3] = {c->dictLast.as<uint8_t>(), c->dictPrevH.as<uint8_t>(), c->dictPrevX.as<uint8_t>()};
        const uint64_t off[3] = {0, lastBytes, lastBytes + slotBytes}, len[3] = {lastBytes, slotBytes, slotBytes};
        for (int k = 0; k < 3; k++)
          if ((r = hipMemcpyAsync(save ? snap + off[k] : t[k], save ? t[k] : snap + off[k], len[k],
                                  hipMemcpyDeviceToDevice, s)))
            return r;
        return hipSuccess;
      };
      if ((!mode.legacy && (e = tables(true))) || (e = hipMemsetAsync(P.ivCount, 0, nb * 4, s)))
        return c->fail(SZ4_E_DEVICE, "dictionary tables", e);
      A.ph = c->dictPH.as<uint16_t>();
      A.pe = c->dictPE.as<uint16_t>();
      A.keysA = c->dictKeys.as<uint64_t>();
      A.keysB = c->dictKeys.as<uint64_t>() + dict_sort_keys_max();
      A.temp = c->dictTemp.p;
      A.tempBytes = c->dictTempBytes;
      A.lzMasks = c->dictLz.as<uint32_t>();
      A.scBits = c->dictSc.as<uint64_t>();
      A.runTab = c->dictRuns.as<uint2>();
      A.runFlag = reinterpret_cast<uint32_t*>(A.runTab + (staged / 64 + 2));
      for (uint32_t round = 0;; round++) {
        A.buildRuns = round == 0;
        A.guess = round == 0 && !c->dictNoGuess;
        if (round > 0 && ((!mode.legacy && (e = tables(false))) || (e = hipMemsetAsync(P.longFlag, 0, nb * 4, s))))
          return c->fail(SZ4_E_DEVICE, "dictionary tables", e);
        if (launch_dict_parallel(A, s)) return c->fail(SZ4_E_DEVICE, "dictionary kernels");
        int st = 0;
        if ((e = hipMemcpyAsync(&st, P.status, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
          return c->fail(SZ4_E_DEVICE, "dictionary rounds", e);
        if (c->dictRounds != ~0u) c->dictRounds = std::max(c->dictRounds, round + 1);  // sticky over the call's chunks
        if (!(st & (kStPrepRound | kStInvariant))) break;
        if ((e = hipMemsetAsync(P.status, 0, 4, s))) return c->fail(SZ4_E_DEVICE, "dictionary rounds", e);
        // every round settles a longer prefix, so this is a safety net, not a path: the in-order replay
        if ((st & kStInvariant) || round + 1 >= (c->dictMaxRounds ? c->dictMaxRounds : dict_round_cap(maxBlock))) {
          if ((!mode.legacy && (e = tables(false))) || (e = hipMemsetAsync(P.longFlag, 0, nb * 4, s)))
            return c->fail(SZ4_E_DEVICE, "dictionary tables", e);
          launch_dict(A, s);
          c->dictRounds = ~0u;
          break;
        }
      }
    }
    mark(c, 2, s);
    mark(c, 3, s);
    mark(c, 4, s);
    if (c->stopAfter == 3) return stop_here(c, s);
  }
  // greedy/lazy levels: k_lazy_check verifies the shortcut intervals k_runs assumed; a corrected block
  // needs another sort/find/walk round (each round checks a longer prefix of it)
  for (uint32_t round = 0; !dictMode; round++) {
    if (maxChain > 0) {
      // k_find_sorted writes every target (shortcut-interval targets "unresolved", for pass 2); its
      // marker bits are OR-ed in
      if ((e = hipMemsetAsync(P.longBits, 0, c->pipe.plan.blocks.back().end / 8 + 8, s)))
        return c->fail(SZ4_E_DEVICE, "clear matches", e);
    }
    mark(c, 2, s);
    if (maxChain > 0) launch_find(1, P, s);
    mark(c, 3, s);
    if (c->stopAfter == 2) return stop_here(c, s);
    if (maxChain > 0) launch_find(2, P, s);
    mark(c, 4, s);
    if (c->stopAfter == 3) return stop_here(c, s);
    launch_prep(P, s);
    if (maxChain == 0 || maxChain > (uint32_t)kLazyMax) break;
    // greedy/lazy: the reference's skip bookkeeping in parallel over the assumed shortcut intervals, which
    // k_lazy_check / k_lazy_correct then compare with the ones the searches imply
    launch_lazy(P, s);
    int st = 0;
    if ((e = hipMemcpyAsync(&st, P.status, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
      return c->fail(SZ4_E_DEVICE, "prep", e);
    if (!(st & 2)) break;
    if (round > 2 * kMaxIv + 2) return c->fail(SZ4_E_DEVICE, "shortcut intervals did not settle");
    if ((e = hipMemsetAsync(P.status, 0, 4, s)) || (e = hipMemsetAsync(P.longFlag, 0, nb * 4, s)))
      return c->fail(SZ4_E_DEVICE, "prep", e);
  }
  launch_parse(P, s);
  mark(c, 5, s);
  if (c->stopAfter == 4) return stop_here(c, s);
  launch_emit(P, s);
  mark(c, 6, s);
  if ((e = hipGetLastError())) return c->fail(SZ4_E_DEVICE, "kernel launch", e);
  c->lastBlocks = nb;
  if (!finish) return SZ4_OK;
  return pipeline_finish(c, hdr, hdrLen, endMark, out, outCap, outSize, s);
}

// the frame size and device status of the pipeline enqueued last on s; header and end mark around it
int pipeline_finish(sz4_ctx* c, const uint8_t* hdr, uint64_t hdrLen, bool endMark, uint8_t* out, uint64_t outCap,
                    uint64_t* outSize, hipStream_t s)
{
  const uint32_t nb = (uint32_t)c->pipe.plan.blocks.size();
  hipError_t e;
  uint64_t total = 0;
  int status = 0;
  if ((e = hipMemcpyAsync(&total, c->pipe.offsets.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(&status, c->pipe.status.p, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
    return c->fail(SZ4_E_DEVICE, "pipeline", e);
  if (status & kStInvariant) return c->fail(SZ4_E_DEVICE, "device invariant failed (walk slots / token capacity)");
  const uint64_t size = hdrLen + total + (endMark ? 4 : 0);
  if (size > outCap) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
  if (hdrLen && (e = hipMemcpyAsync(out, hdr, hdrLen, hipMemcpyHostToDevice, s)))
    return c->fail(SZ4_E_DEVICE, "header", e);
  if (endMark && (e = hipMemsetAsync(out + hdrLen + total, 0, 4, s))) return c->fail(SZ4_E_DEVICE, "end mark", e);
  if ((e = hipStreamSynchronize(s))) return c->fail(SZ4_E_DEVICE, "finish", e);
  if (c->timing)
    for (int i = 0; i < kStages; i++) hipEventElapsedTime(&c->stageMs[i], c->ev[i], c->ev[i + 1]);
  *outSize = size;
  return SZ4_OK;
}

// ---- decoder (the reference's smallz4cat) ----------------------------------------------------
// Index and sizes passes: every block's output offset.  A legacy frame ends after its first block
// shorter than 8 MiB (smallz4cat.c:325-327), so a malformed tail after that block does not matter.
// *keep = blocks to decode, *total = decoded bytes.
int unlz4_plan(sz4_ctx* c, const uint8_t* f, uint64_t n, uint64_t* total, uint32_t* keep, hipStream_t s)
{
  hipError_t e;
  uint64_t maxBlocks = std::min<uint64_t>(n / 5 + 2, 1u << 16);  // a block takes >= 5 frame bytes
  uint64_t meta[5] = {0, 0, 0, 0, 0};
  for (;;) {
    if ((e = c->unBlk.reserve(maxBlocks * sizeof(UnBlock) + 64)) || (e = c->unMeta.reserve(64)))
      return c->fail(SZ4_E_NOMEM, "decoder scratch", e);
    // the parallel index (its scratch is about 3n / 8 bytes); the one-lane walk when that does not fit.  Under a
    // device bound it is tried only if it fits without releasing other buffers (it is optional: ADVICE r05)
    const uint64_t ixBytes = unlz4_ix_scratch_bytes(n);
    if (!c->unIndexSerial && c->unIx.fits(ixBytes) && c->unIx.reserve(ixBytes) == hipSuccess)
      launch_unlz4_index_par(f, n, c->unIx.p, c->unBlk.as<UnBlock>(), maxBlocks, c->unMeta.as<uint64_t>(), s);
    else
      launch_unlz4_index(f, n, c->unBlk.as<UnBlock>(), maxBlocks, c->unMeta.as<uint64_t>(), s);
    if ((e = hipMemcpyAsync(meta, c->unMeta.p, sizeof meta, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
      return c->fail(SZ4_E_DEVICE, "frame index", e);
    // the index scratch is dead once its result is read: kept for the next call, but releasable by a
    // growing reservation of this one (the split buffers, the output)
    c->unIx.lastGen = 0;
    if (meta[1] != 2) break;
    maxBlocks = n / 5 + 2;
  }
  const uint32_t nb = (uint32_t)meta[0];
  c->unIndexParallel = meta[3] == 1;
  c->hUn.resize(nb);
  c->unSplit = false;
  // split mode needs about twice the per-block decoder's scratch (the u32 image, the sub-segment lists):
  // when it does not fit, or its 31-bit image cannot address the output, the frame decodes block by block
  auto blockwise = [&]() {
    for (DevBuf* b : {&c->unSubs, &c->unMasks, &c->unImage}) b->release();
    const int mode = c->unSplitMode;
    c->unSplitMode = 0;
    const int r = unlz4_plan(c, f, n, total, keep, s);
    c->unSplitMode = mode;
    return r;
  };
  if (nb) {
    // split mode when a block is large (one wavefront per block would leave most of the chip idle); the
    // index reports the longest payload, so block-wise decoding reads the records back only after sizes
    const uint64_t maxLen = meta[4];
    c->unSplit = c->unSplitMode == 1 || (c->unSplitMode != 0 && maxLen >= kUnSplitMin);
    if (c->unSplit && ((e = hipMemcpyAsync(c->hUn.data(), c->unBlk.p, nb * sizeof(UnBlock), hipMemcpyDeviceToHost, s)) ||
                       (e = hipStreamSynchronize(s))))
      return c->fail(SZ4_E_DEVICE, "frame index", e);
  }
  if (nb && c->unSplit) {
    c->hSub.clear();
    for (uint32_t b = 0; b < nb; b++) {
      UnBlock& B = c->hUn[b];
      B.subFirst = (uint32_t)c->hSub.size();
      B.subCount = (B.len + kUnSub - 1) / kUnSub;
      for (uint32_t k = 0; k < B.subCount; k++) c->hSub.push_back(UnSub{b, k});
    }
    const uint32_t nsub = (uint32_t)c->hSub.size();
    if ((e = c->unSeq.reserve((uint64_t)nsub * 2 * kUnSubCap * sizeof(uint4) + 64)) ||
        (e = c->unSubs.reserve((uint64_t)nsub * sizeof(UnSub) + 64)) ||
        (e = c->unMasks.reserve((uint64_t)nsub * kUnAuxWords * 4 + 64))) {
      c->unSeq.release();
      return blockwise();
    }
    if ((e = hipMemcpyAsync(c->unBlk.p, c->hUn.data(), nb * sizeof(UnBlock), hipMemcpyHostToDevice, s)) ||
        (e = hipMemcpyAsync(c->unSubs.p, c->hSub.data(), nsub * sizeof(UnSub), hipMemcpyHostToDevice, s)))
      return c->fail(SZ4_E_DEVICE, "decoder plan", e);
    launch_unlz4_split_sizes(f, n, c->unBlk.as<UnBlock>(), nb, c->unSubs.as<UnSub>(), nsub, c->unSeq.as<uint4>(),
                             c->unMasks.as<uint32_t>(), s);
    if ((e = hipMemcpyAsync(c->hUn.data(), c->unBlk.p, nb * sizeof(UnBlock), hipMemcpyDeviceToHost, s)) ||
        (e = hipStreamSynchronize(s)))
      return c->fail(SZ4_E_DEVICE, "block sizes", e);
  } else if (nb) {
    if ((e = c->unSeq.reserve(unlz4_seq_entries(n, nb) * sizeof(uint4) + 64)))
      return c->fail(SZ4_E_NOMEM, "decoder sequences", e);
    launch_unlz4_sizes(f, n, c->unBlk.as<UnBlock>(), nb, c->unSeq.as<uint4>(), s);
    if ((e = hipMemcpyAsync(c->hUn.data(), c->unBlk.p, nb * sizeof(UnBlock), hipMemcpyDeviceToHost, s)) ||
        (e = hipStreamSynchronize(s)))
      return c->fail(SZ4_E_DEVICE, "block sizes", e);
  }
  uint64_t w = 0;
  uint32_t k = 0;
  bool ended = false;
  while (k < nb) {
    UnBlock& b = c->hUn[k++];
    if (b.size == kNone) return c->fail(SZ4_E_CORRUPT, "malformed LZ4 block");
    b.dst = w;
    w += b.size;
    if (meta[2] && b.size < kBlockMaxLegacy) {
      ended = true;
      break;
    }
  }
  if (meta[1] != 0 && !ended) return c->fail(SZ4_E_CORRUPT, "invalid or truncated LZ4 frame");
  // the split image addresses output bytes with 31 bits: a larger output decodes block by block
  if (c->unSplit && w >= (uint64_t)kUnRef) {
    c->unSeq.release();
    return blockwise();
  }
  if (c->unSplit && ((e = c->unImage.reserve(w * 4 + 64)) || (e = c->unFlags.reserve(64)))) {
    c->unSeq.release();
    return blockwise();
  }
  *total = w;
  *keep = k;
  return SZ4_OK;
}

// the device output buffer of the host-buffer decoders (sz4_unlz4, the stream decoder): when it does not fit
// beside a split-mode plan, the frame is planned again block by block (about half the scratch) and the
// reservation retried (the split plan's own check did not count this buffer)
int unlz4_reserve_out(sz4_ctx* c, const uint8_t* f, uint64_t n, uint64_t* total, uint32_t* keep)
{
  hipError_t e = c->unOut.reserve(*total);
  if (e == hipSuccess) return SZ4_OK;
  if (c->unSplit) {
    for (DevBuf* b : {&c->unSubs, &c->unMasks, &c->unImage, &c->unSeq, &c->unIx}) b->release();
    const int mode = c->unSplitMode;
    c->unSplitMode = 0;
    const int r = unlz4_plan(c, f, n, total, keep, nullptr);
    c->unSplitMode = mode;
    if (r) return r;
    e = c->unOut.reserve(*total);
    if (e == hipSuccess) return SZ4_OK;
  }
  return c->fail(SZ4_E_NOMEM, "output", e);
}

int unlz4_decode(sz4_ctx* c, const uint8_t* f, uint64_t n, const uint8_t* dict, uint64_t dl, uint8_t* out, uint32_t keep,
                 hipStream_t s)
{
  if (!keep) return SZ4_OK;
  hipError_t e;
  if (c->unSplit) {
    // split mode: the u32 image of the output, its references resolved, then packed into `out`
    const UnBlock& lastB = c->hUn[keep - 1];
    const uint64_t total = lastB.dst + lastB.size;
    const uint32_t nsub = lastB.subFirst + lastB.subCount;
    if (c->unImage.cap < total * 4 + 64 || c->unFlags.cap < 64) return c->fail(SZ4_E_NOMEM, "decoder image");
    uint32_t* flag = c->unFlags.as<uint32_t>();
    if ((e = hipMemcpyAsync(c->unBlk.p, c->hUn.data(), keep * sizeof(UnBlock), hipMemcpyHostToDevice, s)))
      return c->fail(SZ4_E_DEVICE, "decoder plan", e);
    launch_unlz4_split_decode(f, n, c->unBlk.as<UnBlock>(), c->unSubs.as<UnSub>(), nsub, c->unSeq.as<uint4>(),
                              c->unImage.as<uint32_t>(), dict, dl, s);
    // the pack follows every reference chain to its byte (each hop lands in an earlier sub-segment): no
    // host round trip between passes; unResolvePasses reports the longest chain
    if ((e = hipMemsetAsync(flag, 0, 4, s))) return c->fail(SZ4_E_DEVICE, "decoder resolve", e);
    launch_unlz4_pack(c->unImage.as<uint32_t>(), total, out, flag, s);
    uint32_t hops = 0;
    if ((e = hipGetLastError()) || (e = hipMemcpyAsync(&hops, flag, 4, hipMemcpyDeviceToHost, s)) ||
        (e = hipStreamSynchronize(s)))
      return c->fail(SZ4_E_DEVICE, "decode", e);
    c->unResolvePasses = hops;
    return SZ4_OK;
  }
  const uint64_t flagBytes = ((uint64_t)keep + 2) * 4;
  if ((e = c->unFlags.reserve(flagBytes + 64))) return c->fail(SZ4_E_NOMEM, "decoder flags", e);
  uint32_t* flags = c->unFlags.as<uint32_t>();
  uint32_t status = 0;
  if ((e = hipMemcpyAsync(c->unBlk.p, c->hUn.data(), keep * sizeof(UnBlock), hipMemcpyHostToDevice, s)) ||
      (e = hipMemsetAsync(flags, 0, flagBytes, s)))
    return c->fail(SZ4_E_DEVICE, "decoder plan", e);
  launch_unlz4_blocks(f, n, c->unBlk.as<UnBlock>(), keep, c->unSeq.as<uint4>(), out, dict, dl, flags, s);
  if ((e = hipGetLastError()) || (e = hipMemcpyAsync(&status, flags + keep, 4, hipMemcpyDeviceToHost, s)) ||
      (e = hipStreamSynchronize(s)))
    return c->fail(SZ4_E_DEVICE, "decode", e);
  if (status & 2u) return c->fail(SZ4_E_DEVICE, "decoder wait timed out");
  if (status) return c->fail(SZ4_E_DEVICE, "decoded length differs from the size pass");
  return SZ4_OK;
}


// ---- stream path: smallz4::lz4 over GET_BYTES / SEND_BYTES in bounded memory --------------------
// The input is compressed in chunks of whole blocks (4 MiB, legacy 8 MiB; c->streamChunk bytes per
// chunk).  A chunk is staged as [carried bytes | new bytes]: the carried bytes are the previous
// chunk's last 64..128 KiB (the reference keeps the last MaxDistance bytes, smallz4.h:798-805), so
// the chunk's first block sees exactly the window the reference's does.  The state a block takes
// from its predecessor -- the lookback cut (smallz4.h:614-624) and the positions the same-letter
// shortcut left out of the chains -- comes along as the previous block's final intervals in the
// ghost slot; dictionary mode carries the reference's hash table and chains.  The device footprint
// is fixed by the chunk size, whatever the input length.  Three streams overlap the chunks: while the
// compute stream runs chunk k+1, chunk k comes down on the download stream and goes to sendBytes, and
// chunk k+2 is pulled through getBytes and goes up on the upload stream (two staging and two output
// slots).  Both callbacks run on the caller's thread.
constexpr uint64_t kCarryMax = 2 * 65536;

struct MemSource {
  const uint8_t* p;
  uint64_t n, at;
};
struct MemSink {
  uint8_t* p;
  uint64_t cap, n;
};
size_t mem_get(void* data, size_t want, void* user)
{
  MemSource* m = static_cast<MemSource*>(user);
  const uint64_t k = std::min<uint64_t>(want, m->n - m->at);
  if (k) memcpy(data, m->p + m->at, k);
  m->at += k;
  return (size_t)k;
}
void mem_send(const void* data, size_t n, void* user)
{
  MemSink* m = static_cast<MemSink*>(user);
  if (n && m->n + n <= m->cap) memcpy(m->p + m->n, data, n);
  m->n += n;
}

// the reference's output call pattern for a run of blocks: four 1-byte calls for the size word, then
// the payload, also when it is empty (smallz4.h:770-780)
void send_blocks(const uint8_t* f, uint64_t n, sz4_send_bytes send, void* user)
{
  uint64_t pos = 0;
  while (pos + 4 <= n) {
    uint32_t word = 0;
    memcpy(&word, f + pos, 4);
    for (int k = 0; k < 4; k++) send(f + pos + k, 1, user);
    pos += 4;
    const uint32_t bytes = word & 0x7FFFFFFFu;
    send(f + pos, bytes, user);
    pos += bytes;
  }
}

// grows pinned buffer b to at least `bytes`, keeping its first `keep` bytes
hipError_t grow_pinned(HostBuf& b, uint64_t bytes, uint64_t keep)
{
  if (bytes <= b.cap) return hipSuccess;
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return e;
  if (keep && b.p) memcpy(p, b.p, keep);
  if (b.p) hipHostFree(b.p);
  b.p = p;
  b.cap = bytes;
  return hipSuccess;
}

// reads up to `want` bytes through getBytes, 64 KiB per call (the reference's BufferSize), into pinned
// buffer b, which grows as it fills (a small input pins little); *eof is set once getBytes returns 0.
// A getBytes that returns more than it was asked for is an error (*bad)
uint64_t pull(HostBuf& b, sz4_get_bytes get, void* user, uint64_t want, bool* eof, hipError_t* err, bool* bad)
{
  uint64_t got = 0;
  while (got < want && !*eof) {
    if (got == b.cap && (*err = grow_pinned(b, std::min<uint64_t>(want, std::max<uint64_t>(4 * b.cap, 1u << 20)), got)))
      return got;
    const uint64_t ask = std::min<uint64_t>(65536, std::min<uint64_t>(want, b.cap) - got);
    const size_t k = get(b.as<uint8_t>() + got, (size_t)ask, user);
    if (k > ask) {
      *bad = true;
      *eof = true;
      return got;
    }
    if (k == 0) *eof = true;
    got += k;
  }
  return got;
}

// one chunk of the stream: [pre carried bytes | n new bytes] in stagedS[slot]
struct StreamChunk {
  uint64_t pre = 0, n = 0;
  bool first = false;
  uint64_t shift() const { return (pre + n - 65536) / 65536 * 65536; }  // carry: [shift, pre + n) moves to 0
  uint64_t nextPre() const { return pre + n - shift(); }
};

// drains the stream path's streams before an early return (nothing may still run on its buffers)
struct StreamDrain {
  sz4_ctx* c;
  ~StreamDrain()
  {
    for (hipStream_t x : {c->upStream, c->stream, c->downStream})
      if (x) hipStreamSynchronize(x);
  }
};

// header and blocks of the stream; the end mark is stream_compress's
int stream_compress_body(sz4_ctx* c, sz4_get_bytes get, sz4_send_bytes send, uint32_t maxChain, const uint8_t* dict,
                         uint64_t dictLen, int legacy, void* user, void* out)
{
  hipError_t e;
  for (hipStream_t* x : {&c->stream, &c->upStream, &c->downStream})
    if (!*x && (e = hipStreamCreateWithFlags(x, hipStreamNonBlocking))) return c->fail(SZ4_E_DEVICE, "stream", e);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t* x : {&c->evUp[k], &c->evDone[k]})
      if (!*x && (e = hipEventCreateWithFlags(x, hipEventDisableTiming))) return c->fail(SZ4_E_DEVICE, "event", e);
  const uint64_t bs = legacy ? kBlockMaxLegacy : kBlockMax;
  const uint64_t chunk = std::max<uint64_t>(bs, c->streamChunk / bs * bs);
  const bool dictMode = dictLen != 0;
  // header (smallz4.h:478-496)
  if (legacy) send(kLegacyMagic, sizeof kLegacyMagic, out);
  else send(kFrameHeader, sizeof kFrameHeader, out);
  StreamDrain drain{c};
  bool eof = false, bad = false;
  hipError_t he = hipSuccess;
  StreamChunk ch[2];
  ch[0].n = pull(c->hostIn[0], get, user, chunk, &eof, &he, &bad);
  if (he) return c->fail(SZ4_E_NOMEM, "pinned host buffers", he);
  if (bad) return c->fail(SZ4_E_ARG, "getBytes returned more bytes than asked for");
  // dictionary: the staged stream starts with the reference's data buffer, a 65535-byte prefix (the
  // dictionary's last bytes, zero-padded in front) (smallz4.h:554-571)
  RunMode mode;
  mode.dictBack = dictMode ? (int64_t)std::min<uint64_t>(dictLen, kWindow) : -1;
  mode.legacy = legacy;
  ch[0].pre = dictMode && ch[0].n ? kWindow : 0;
  ch[0].first = true;
  if (ch[0].n) {
    // device buffers fixed by the chunk size (by the input when it is shorter than a chunk); the
    // scratch is sized once for the steady-state chunk shape, so no buffer moves mid-stream
    const uint64_t span = eof ? ch[0].n : chunk;
    const uint64_t stage = (eof ? ch[0].pre : kCarryMax) + span + kPad;
    if ((e = c->stagedS[0].reserve(stage)) || (!eof && (e = c->stagedS[1].reserve(stage))) ||
        (e = c->chunkOut[0].reserve(sz4_lz4_bound(span, legacy))) ||
        (!eof && (e = c->chunkOut[1].reserve(sz4_lz4_bound(span, legacy)))))
      return c->fail(SZ4_E_NOMEM, "stream staging", e);
    StreamChunk worst;
    worst.pre = eof ? ch[0].pre : kCarryMax - 1;
    worst.n = span;
    worst.first = eof;
    c->pipe.plan.build_stream(worst.pre, worst.n, worst.first, legacy, dictMode);
    if (int r = reserve_all(c, worst.pre + worst.n + kPad)) return r;
  }
  if (dictMode && ch[0].n) {
    std::vector<uint8_t> prefix(kWindow, 0);
    const uint64_t k = std::min<uint64_t>(dictLen, kWindow);
    memcpy(prefix.data() + kWindow - k, dict + dictLen - k, k);
    if ((e = hipMemcpy(c->stagedS[0].p, prefix.data(), kWindow, hipMemcpyHostToDevice)))
      return c->fail(SZ4_E_DEVICE, "upload", e);
  }
  // chunk k -> slot k & 1: upload on the copy stream (after chunk k-2 let go of the slot), with the
  // previous chunk's carried bytes in front
  auto upload = [&](uint32_t k) -> int {
    const uint32_t sl = k & 1;
    const StreamChunk& x = ch[sl];
    uint8_t* dst = c->stagedS[sl].as<uint8_t>();
    if (k >= 2 && (e = hipStreamWaitEvent(c->upStream, c->evDone[sl], 0))) return c->fail(SZ4_E_DEVICE, "upload", e);
    if ((e = hipMemcpyAsync(dst + x.pre, c->hostIn[sl].p, x.n, hipMemcpyHostToDevice, c->upStream)) ||
        (k >= 1 && (e = hipMemcpyAsync(dst, c->stagedS[sl ^ 1].as<uint8_t>() + ch[sl ^ 1].shift(), x.pre,
                                       hipMemcpyDeviceToDevice, c->upStream))) ||
        (e = hipMemsetAsync(dst + x.pre + x.n, 0, kPad, c->upStream)) || (e = hipEventRecord(c->evUp[sl], c->upStream)))
      return c->fail(SZ4_E_DEVICE, "upload", e);
    return SZ4_OK;
  };
  // enqueue chunk k's pipeline on the compute stream (returns with the kernels in flight)
  auto compute = [&](uint32_t k) -> int {
    const uint32_t sl = k & 1;
    const StreamChunk& x = ch[sl];
    mode.ghost = !legacy && !x.first && !dictMode;
    c->pipe.plan.build_stream(x.pre, x.n, x.first, legacy, dictMode);
    if (int r = reserve_all(c, x.pre + x.n + kPad)) return r;
    if ((e = hipStreamWaitEvent(c->stream, c->evUp[sl], 0))) return c->fail(SZ4_E_DEVICE, "chunk", e);
    uint64_t unused = 0;
    if (int r = run_pipeline(c, mode, maxChain, c->stagedS[sl].as<uint8_t>(), nullptr, 0, false,
                             c->chunkOut[sl].as<uint8_t>(), c->chunkOut[sl].cap, &unused, c->stream, false))
      return r;
    if ((e = hipEventRecord(c->evDone[sl], c->stream))) return c->fail(SZ4_E_DEVICE, "chunk", e);
    return SZ4_OK;
  };
  // chunk k's frame size; the state its successor takes: the last block's final shortcut intervals
  // (the ghost slot) and dictionary mode's table position
  auto finish = [&](uint32_t k, uint64_t* size) -> int {
    const uint32_t sl = k & 1;
    const StreamChunk& x = ch[sl];
    if (int r = pipeline_finish(c, nullptr, 0, false, c->chunkOut[sl].as<uint8_t>(), c->chunkOut[sl].cap, size, c->stream))
      return r;
    const uint64_t shift = x.shift();
    const uint32_t nb = (uint32_t)c->pipe.plan.blocks.size();
    if (!legacy && !dictMode) {
      uint32_t cnt = 0;
      if ((e = hipMemcpyAsync(&cnt, c->pipe.ivCount.as<uint32_t>() + (nb - 1), 4, hipMemcpyDeviceToHost, c->stream)) ||
          (e = hipStreamSynchronize(c->stream)))
        return c->fail(SZ4_E_DEVICE, "intervals", e);
      std::vector<Interval> iv(cnt);
      if (cnt && ((e = hipMemcpyAsync(iv.data(), c->pipe.iv.as<Interval>() + (uint64_t)(nb - 1) * kMaxIv, cnt * sizeof(Interval),
                                      hipMemcpyDeviceToHost, c->stream)) || (e = hipStreamSynchronize(c->stream))))
        return c->fail(SZ4_E_DEVICE, "intervals", e);
      c->ghostIv.clear();
      for (Interval y : iv) {
        if (y.hi <= shift) continue;
        y.lo = std::max(y.lo, shift) - shift;
        y.hi -= shift;
        y.a = y.a >= shift ? y.a - shift : 0;
        c->ghostIv.push_back(y);
      }
    }
    if (dictMode) {
      mode.cont = legacy ? 0u : 1u;
      mode.shift = (uint32_t)shift;
      mode.low0 = (uint32_t)(x.nextPre() - kWindow);
    }
    return SZ4_OK;
  };
  // the next chunk's bytes: [previous chunk's carry | new bytes]
  auto next_chunk = [&](uint32_t k) -> bool {
    const uint32_t sl = k & 1;
    if (eof) return false;
    if (k >= 2 && (e = hipEventSynchronize(c->evUp[sl]))) {  // the pinned buffer's previous upload
      c->fail(SZ4_E_DEVICE, "upload", e);
      return false;
    }
    ch[sl].n = pull(c->hostIn[sl], get, user, chunk, &eof, &he, &bad);
    ch[sl].pre = ch[sl ^ 1].nextPre();
    ch[sl].first = false;
    return ch[sl].n != 0 && !he && !bad;
  };
  if (!ch[0].n) return SZ4_OK;
  if (int r = upload(0)) return r;
  if (int r = compute(0)) return r;
  bool have = next_chunk(1);
  if (he) return c->fail(SZ4_E_NOMEM, "pinned host buffers", he);
  if (bad) return c->fail(SZ4_E_ARG, "getBytes returned more bytes than asked for");
  if (have)
    if (int r = upload(1)) return r;
  // SZ4_STREAM_PROFILE=1: where the caller's thread spends its time, per phase, on stderr
  const bool prof = getenv("SZ4_STREAM_PROFILE") != nullptr;
  double tp[6] = {0, 0, 0, 0, 0, 0};
  auto now = []() { return std::chrono::steady_clock::now(); };
  auto lap = [&](std::chrono::steady_clock::time_point& t, int i) {
    const auto u = now();
    tp[i] += std::chrono::duration<double>(u - t).count();
    t = u;
  };
  for (uint32_t k = 0;; k++) {
    const uint32_t sl = k & 1;
    uint64_t size = 0;
    auto t = now();
    if (int r = finish(k, &size)) return r;
    lap(t, 0);
    if (have)
      if (int r = compute(k + 1)) return r;  // the GPU goes on with chunk k+1 ...
    lap(t, 1);
    // ... while chunk k comes down (its copy overlaps the read of chunk k+2) and goes out, and chunk
    // k+2 is read and goes up
    if ((e = grow_pinned(c->hostOut[sl], std::max<uint64_t>(size, 1), 0))) return c->fail(SZ4_E_NOMEM, "pinned host buffers", e);
    if ((e = hipMemcpyAsync(c->hostOut[sl].p, c->chunkOut[sl].p, size, hipMemcpyDeviceToHost, c->downStream)))
      return c->fail(SZ4_E_DEVICE, "download", e);
    const bool more = have;
    if (more) {
      have = next_chunk(k + 2);
      if (he) return c->fail(SZ4_E_NOMEM, "pinned host buffers", he);
      if (bad) return c->fail(SZ4_E_ARG, "getBytes returned more bytes than asked for");
      lap(t, 4);
      if (have)
        if (int r = upload(k + 2)) return r;
      lap(t, 5);
    }
    if ((e = hipStreamSynchronize(c->downStream))) return c->fail(SZ4_E_DEVICE, "download", e);
    lap(t, 2);
    send_blocks(c->hostOut[sl].as<uint8_t>(), size, send, out);
    lap(t, 3);
    if (!more) break;
  }
  if (prof)
    fprintf(stderr, "sz4 stream: finish-wait %.3f s, enqueue %.3f s, download %.3f s, sendBytes %.3f s, getBytes %.3f s, "
            "upload-enqueue %.3f s\n", tp[0], tp[1], tp[2], tp[3], tp[4], tp[5]);
  return SZ4_OK;
}

// smallz4::lz4 over the callbacks.  A callback's exception (a C++ caller's sendBytes may throw) leaves
// through here after the streams have drained; an allocation failure becomes SZ4_E_NOMEM
int stream_compress(sz4_ctx* c, sz4_get_bytes get, sz4_send_bytes send, uint32_t maxChain, const uint8_t* dict,
                    uint64_t dictLen, int legacy, void* user, void* sinkUser = nullptr)
{
  c->dictRounds = 0;  // sz4_dict_rounds reports this call's chunks
  try {
    void* out = sinkUser ? sinkUser : user;
    const int r = stream_compress_body(c, get, send, maxChain, dict, dictLen, legacy, user, out);
    static const uint8_t zero[4] = {0, 0, 0, 0};
    if (r == SZ4_OK && !legacy) send(zero, 4, out);  // end mark (smallz4.h:807-812)
    return r;
  } catch (const std::bad_alloc&) {
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
}

// ---- decoder stream path: unlz4_userPtr over GET_BYTE / SEND_BYTES in bounded memory -----------
// getByte is called exactly where the reference calls it on a valid frame (header, size words,
// payloads, checksums; a legacy frame ends after its first block that decodes to less than 8 MiB,
// smallz4cat.c:325-327).  Blocks are pulled until about c->streamChunk / 2 frame bytes are queued,
// rewrapped as a plain frame (smallz4's header, the blocks, an end mark; checksums dropped) and
// decoded on the GPU with the last 64 KiB of output (at first the dictionary's) as its history.
// sendBytes receives the output in 64 KiB pieces and the remainder at the end -- the reference's
// flush points (smallz4cat.c:249-253, 358-359).
uint64_t legacy_block_length(const uint8_t* p, uint64_t len)
{
  uint64_t r = 0, w = 0;
  while (r < len) {
    const uint8_t tok = p[r++];
    uint64_t lits = tok >> 4, ml = 4 + (tok & 15);
    uint8_t x;
    if (lits == 15) do { if (r >= len) return w; x = p[r++]; lits += x; } while (x == 255);
    r += lits;
    w += lits;
    if (r >= len) break;
    r += 2;
    if (ml == 19) do { if (r >= len) return w; x = p[r++]; ml += x; } while (x == 255);
    w += ml;
  }
  return w;
}

int stream_decompress(sz4_ctx* c, sz4_get_byte get, sz4_send_out send, const uint8_t* dict, uint64_t dictLen, void* user)
{
  uint32_t sig = 0;
  for (int k = 0; k < 4; k++) sig |= (uint32_t)get(user) << (8 * k);
  const bool modern = sig == 0x184D2204u, legacy = sig == 0x184C2102u;
  if (!modern && !legacy) return c->fail(SZ4_E_CORRUPT, "invalid signature");
  bool blockSum = false, contentSum = false;
  if (modern) {
    const uint8_t flags = get(user);
    if ((flags >> 6) != 1) return c->fail(SZ4_E_CORRUPT, "only LZ4 file format version 1 supported");
    blockSum = (flags & 16) != 0;
    contentSum = (flags & 4) != 0;
    int skip = 1 + ((flags & 8) ? 8 : 0) + ((flags & 1) ? 4 : 0) + 1;
    while (skip--) get(user);
  }
  std::vector<uint8_t> hist;  // the last <= 64 KiB before the next chunk's output
  if (dictLen) hist.assign(dict + (dictLen - std::min<uint64_t>(dictLen, 65536)), dict + dictLen);
  std::vector<uint8_t> frame, out, pend;  // pend: output not yet flushed (< 64 KiB)
  const uint8_t* hdr = kFrameHeader;
  const uint64_t budget = std::max<uint64_t>(c->streamChunk / 2, 1u << 20);
  auto decode = [&]() -> int {
    if (frame.size() <= 7) return SZ4_OK;
    for (int k = 0; k < 4; k++) frame.push_back(0);  // end mark
    // one upload, one plan (its block sizes give the output length), one decode, one download
    hipError_t e;
    const uint64_t dl = hist.size(), fl = frame.size();
    if ((e = c->unFrame.reserve(fl + 64)) || (e = c->unDict.reserve(dl + 64))) return c->fail(SZ4_E_NOMEM, "staging", e);
    if ((e = hipMemcpy(c->unFrame.p, frame.data(), fl, hipMemcpyHostToDevice)) ||
        (dl && (e = hipMemcpy(c->unDict.p, hist.data(), dl, hipMemcpyHostToDevice))))
      return c->fail(SZ4_E_DEVICE, "upload", e);
    uint64_t size = 0;
    uint32_t keep = 0;
    if (int r = unlz4_plan(c, c->unFrame.as<uint8_t>(), fl, &size, &keep, nullptr)) return r;
    out.resize(size);
    if (size) {
      if (int r = unlz4_reserve_out(c, c->unFrame.as<uint8_t>(), fl, &size, &keep)) return r;
      if (int r = unlz4_decode(c, c->unFrame.as<uint8_t>(), fl, dl ? c->unDict.as<uint8_t>() : nullptr, dl,
                               c->unOut.as<uint8_t>(), keep, nullptr))
        return r;
      if ((e = hipMemcpy(out.data(), c->unOut.p, size, hipMemcpyDeviceToHost))) return c->fail(SZ4_E_DEVICE, "download", e);
    }
    // new history: the last 64 KiB of (history, output)
    if (size >= 65536) {
      hist.assign(out.end() - 65536, out.end());
    } else {
      hist.insert(hist.end(), out.begin(), out.end());
      if (hist.size() > 65536) hist.erase(hist.begin(), hist.end() - 65536);
    }
    // flush in 64 KiB pieces
    uint64_t at = 0;
    if (!pend.empty()) {
      const uint64_t k = std::min<uint64_t>(65536 - pend.size(), size);
      pend.insert(pend.end(), out.begin(), out.begin() + k);
      at = k;
      if (pend.size() == 65536) {
        send(pend.data(), 65536, user);
        pend.clear();
      }
    }
    for (; at + 65536 <= size; at += 65536) send(out.data() + at, 65536, user);
    pend.insert(pend.end(), out.begin() + at, out.begin() + size);
    frame.assign(hdr, hdr + 7);
    return SZ4_OK;
  };
  frame.assign(hdr, hdr + 7);
  for (;;) {
    uint32_t word = 0;
    for (int k = 0; k < 4; k++) word |= (uint32_t)get(user) << (8 * k);
    const bool packed = legacy || (word & 0x80000000u) == 0;
    if (modern) word &= 0x7FFFFFFFu;
    if (word == 0) break;
    if (legacy && (word & 0x80000000u)) return c->fail(SZ4_E_CORRUPT, "invalid or truncated LZ4 frame");
    // no LZ4 block is larger than a legacy 8 MiB block's worst case: a larger size word is corrupt
    // (the reference would read on until its input ends; this decoder must not reserve gigabytes first)
    if (word > kMaxFrameBlock) return c->fail(SZ4_E_CORRUPT, "block size word larger than any LZ4 block");
    const uint64_t at = frame.size();
    frame.resize(at + 4 + word);
    const uint32_t tagged = word | (packed ? 0u : 0x80000000u);
    memcpy(frame.data() + at, &tagged, 4);
    for (uint32_t k = 0; k < word; k++) frame[at + 4 + k] = get(user);
    if (legacy && packed && legacy_block_length(frame.data() + at + 4, word) < kBlockMaxLegacy) break;
    if (blockSum)
      for (int k = 0; k < 4; k++) get(user);
    if (frame.size() >= budget)
      if (int r = decode()) return r;
  }
  if (contentSum)
    for (int k = 0; k < 4; k++) get(user);
  if (int r = decode()) return r;
  send(pend.data(), (unsigned int)pend.size(), user);
  return SZ4_OK;
}

// input bytes per internal pipeline run of the block entry points (sz4_compress_blocks_device,
// sz4_compress_batch_device): batchChunk; under a device bound about 1/64 of the bound; else, unless set
// explicitly, capped so that the scratch takes at most a quarter of the memory the context could use now
uint64_t piece_bytes(sz4_ctx* c)
{
  uint64_t chunk = c->batchChunk;
  if (c->budget.limit) {
    chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(kPieceFloor, c->budget.limit / 64));
  } else if (!c->batchChunkSet) {
    size_t freeB = 0, totalB = 0;
    hipError_t e = hipMemGetInfo(&freeB, &totalB);
    if (c->budget.testFreeBytes) freeB = c->budget.testFreeBytes;  // tests: a device with this much free memory
    if (e == hipSuccess)
      chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(kPieceFloor, (freeB + c->budget.used) / (4 * kScratchPerByte)));
    else
      (void)hipGetLastError();
  }
  return chunk;
}

// ---- ragged batch API (sz4_compress_batch_device) -------------------------------------------------
// Every non-empty item is one Block of a ragged plan.  Layout in staging: the items of a pipeline run in
// caller order, each at the next multiple of kBatchAlign (64) bytes; k_batch_gather zero-fills the gaps
// and the kPad bytes after the last item.  Why that is safe is DESIGN section 4; in short, every kernel
// addresses a block through its own start / end / low, the bytes past a block's end only ever feed 4-byte
// reads whose excess is masked (in a uniform plan they are the next block's data), the last block still has
// the largest end (the longBits clear), and 64-byte strides give every block at least 64 positions of the
// per-position arrays that double as per-block records (24 bytes per block in `reach` during assembly).
//
// Blocks per pipeline run.  Besides ~50 bytes per staged byte a run needs per BLOCK: its interval slots
// (kMaxIv x 32 = 4352 bytes), and in the shared region per parse or walk segment -- at least one each per
// block -- the larger of the parse's side values (10 KiB), the greedy/lazy replay slots (11 KiB) and the
// token-walk slots (8 KiB), plus ~300 bytes of descriptors: 16 KiB in all.  The cap keeps that at a quarter
// of the piece's per-byte scratch, and at 512 MiB (32768 blocks) for the default piece.
constexpr uint64_t kPerBlockScratch = 16384;
constexpr uint64_t kBatchMaxBlocks = 32768;
uint64_t batch_block_cap(uint64_t piece)
{
  return std::min<uint64_t>(kBatchMaxBlocks, std::max<uint64_t>(64, piece * kScratchPerByte / 4 / kPerBlockScratch));
}

// an item whose window fits the finders' LDS (finish_plan's test: the first segment's window is the whole
// item, and no later segment's reaches further)
bool batch_fits_lds(uint64_t size) { return (size + 8 + 3) / 4 * 4 <= find_lds_bytes(); }

// One pipeline run over the items idx[0..k) (caller indices, ascending, all non-empty): plan, gather,
// compress into out[0, outCap).  bytes[k] receives each item's blockBytes word (size with the 4-byte word,
// top bit = stored); the blocks lie back to back in idx order.  elems (null: every item as it is) holds the
// items' element widths: a run with an item wider than 1 is staged by k_batch_gather_planes, which splits
// every item into its byte planes on the way (the plan is the same: a split item has its item's size).
// filters (null: SZ4_FILTER_BYTES throughout) holds the items' filters: a run with an item of SZ4_FILTER_BITS, of
// any width, is staged by k_batch_gather_bits.
int batch_run(sz4_ctx* c, const std::vector<uint64_t>& idx, const void* const* ptrs, const uint32_t* sizes,
              const uint8_t* elems, const uint8_t* filters, uint32_t maxChain, uint8_t* out, uint64_t outCap,
              std::vector<uint32_t>& bytes, hipStream_t s)
{
  const uint32_t nb = (uint32_t)idx.size();
  bool planes = false, bits = false;
  for (uint32_t k = 0; elems && k < nb; k++) planes |= elems[idx[k]] > 1;
  for (uint32_t k = 0; filters && k < nb; k++) bits |= filters[idx[k]] == SZ4_FILTER_BITS;
  planes |= bits;
  std::vector<BatchItem> items(planes ? 0 : nb);
  std::vector<BatchTyped> typed(planes ? nb : 0);
  std::vector<uint64_t> runSizes(nb);
  for (uint32_t k = 0; k < nb; k++) runSizes[k] = sizes[idx[k]];
  const uint64_t stagedBytes = c->pipe.plan.build_ragged(runSizes) + kPad;
  for (uint32_t k = 0; k < nb; k++) {
    const uint64_t at = c->pipe.plan.blocks[k].start, n = runSizes[k];
    if (planes)
      typed[k] = BatchTyped{(uint64_t)(uintptr_t)ptrs[idx[k]], at, (uint32_t)n,
                            elems[idx[k]] | (bits ? (uint32_t)filters[idx[k]] << kBatchFilterShift : 0u)};
    else items[k] = BatchItem{(uint64_t)(uintptr_t)ptrs[idx[k]], at, n};
  }
  hipError_t e = hipSuccess;
  if (int r = reserve_all(c, stagedBytes)) return r;
  static_assert(sizeof(BatchTyped) == sizeof(BatchItem), "one table size for both gathers");
  if ((e = c->pipe.staged.reserve(stagedBytes)) || (e = c->pipe.batchItems.reserve(nb * sizeof(BatchItem) + 64)))
    return c->fail(SZ4_E_NOMEM, "staging", e);
  // the item table goes up with the plan, on the call's stream; `items` lives until the run has finished
  if ((e = hipMemcpyAsync(c->pipe.batchItems.p, planes ? (const void*)typed.data() : (const void*)items.data(), nb * sizeof(BatchItem),
                          hipMemcpyHostToDevice, s)))
    return c->fail(SZ4_E_DEVICE, "upload items", e);
  if (c->timing) hipEventRecord(c->evGather[0], s);
  if (bits) launch_batch_gather_bits(c->pipe.batchItems.as<BatchTyped>(), nb, c->pipe.staged.as<uint8_t>(), stagedBytes, s);
  else if (planes) launch_batch_gather_planes(c->pipe.batchItems.as<BatchTyped>(), nb, c->pipe.staged.as<uint8_t>(), stagedBytes, s);
  else launch_batch_gather(c->pipe.batchItems.as<BatchItem>(), nb, c->pipe.staged.as<uint8_t>(), stagedBytes, s);
  if (c->timing) hipEventRecord(c->evGather[1], s);
  uint64_t size = 0;
  if (int r = run_pipeline(c, RunMode{}, maxChain, c->pipe.staged.as<uint8_t>(), nullptr, 0, false, out, outCap, &size, s)) return r;
  if (c->timing) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evGather[0], c->evGather[1]) == hipSuccess) c->gatherMs += ms;
  }
  bytes.resize(nb);
  if ((e = hipMemcpy(bytes.data(), c->pipe.blockBytes.p, nb * 4ull, hipMemcpyDeviceToHost)))
    return c->fail(SZ4_E_DEVICE, "block sizes", e);
  return SZ4_OK;
}

// One piece: items [i0, i1) of the call.  At levels above 0 the items whose window fits the finders' LDS and
// the items whose window does not are separate pipeline runs (finish_plan picks the finder per launch: one
// large item would take every small one to the HBM finder).  A piece of one kind compresses straight to
// its place in d_out; a mixed piece compresses both runs into batchTmp and k_batch_move puts every block at
// its caller-order offset -- no payload byte passes through the host.  ext[i] receives item i's bytes in
// d_out (0 for an empty item); the piece occupies d_out[pos, pos + sum of ext).
int batch_piece(sz4_ctx* c, uint64_t i0, uint64_t i1, const void* const* ptrs, const uint32_t* sizes, const uint8_t* elems,
                const uint8_t* filters, uint32_t maxChain, uint8_t* dOut, uint64_t pos, uint32_t* ext, float* stageSum, hipStream_t s)
{
  std::vector<uint64_t> run[2];
  uint64_t bound[2] = {0, 0};
  for (uint64_t i = i0; i < i1; i++) {
    ext[i] = 0;
    if (!sizes[i]) continue;
    const int k = maxChain > 0 && !batch_fits_lds(sizes[i]) ? 1 : 0;
    run[k].push_back(i);
    bound[k] += (uint64_t)sizes[i] + 4;
  }
  auto add_stages = [&]() {
    for (int k = 0; k < kStages; k++) stageSum[k] += c->stageMs[k];
  };
  std::vector<uint32_t> bytes[2];
  if (run[0].empty() || run[1].empty()) {
    const int k = run[0].empty() ? 1 : 0;
    if (run[k].empty()) return SZ4_OK;
    if (int r = batch_run(c, run[k], ptrs, sizes, elems, filters, maxChain, dOut + pos, bound[k], bytes[k], s)) return r;
    add_stages();
    for (size_t j = 0; j < run[k].size(); j++) ext[run[k][j]] = bytes[k][j] & 0x7FFFFFFFu;
    return SZ4_OK;
  }
  hipError_t e;
  if ((e = c->batchTmp.reserve(bound[0] + bound[1] + 64))) return c->fail(SZ4_E_NOMEM, "batch staging", e);
  const uint64_t base[2] = {0, bound[0]};
  for (int k = 0; k < 2; k++) {
    if (int r = batch_run(c, run[k], ptrs, sizes, elems, filters, maxChain, c->batchTmp.as<uint8_t>() + base[k], bound[k], bytes[k],
                          s))
      return r;
    add_stages();
    for (size_t j = 0; j < run[k].size(); j++) ext[run[k][j]] = bytes[k][j] & 0x7FFFFFFFu;
  }
  // every block from its place in its run to its caller-order place, in entries of at most kBatchMoveMax bytes
  std::vector<BatchMove> moves;
  uint64_t from[2] = {base[0], base[1]}, to = pos;
  size_t next[2] = {0, 0};
  for (uint64_t i = i0; i < i1; i++) {
    if (!ext[i]) continue;
    const int k = next[0] < run[0].size() && run[0][next[0]] == i ? 0 : 1;
    next[k]++;
    for (uint64_t o = 0; o < ext[i]; o += kBatchMoveMax)
      moves.push_back(BatchMove{from[k] + o, to + o, std::min<uint64_t>(kBatchMoveMax, ext[i] - o)});
    from[k] += ext[i];
    to += ext[i];
  }
  if ((e = c->batchMoves.reserve(moves.size() * sizeof(BatchMove) + 64))) return c->fail(SZ4_E_NOMEM, "batch moves", e);
  if ((e = hipMemcpyAsync(c->batchMoves.p, moves.data(), moves.size() * sizeof(BatchMove), hipMemcpyHostToDevice, s)))
    return c->fail(SZ4_E_DEVICE, "upload moves", e);
  launch_batch_move(c->batchMoves.as<BatchMove>(), (uint32_t)moves.size(), c->batchTmp.as<uint8_t>(), dOut, s);
  if ((e = hipGetLastError()) || (e = hipStreamSynchronize(s))) return c->fail(SZ4_E_DEVICE, "move blocks", e);
  return SZ4_OK;
}
}  // namespace

extern "C" {

const char* sz4_version(void) { return "1.5"; }

int sz4_create(sz4_ctx** ctx, int device, uint64_t reserve_bytes)
{
  if (!ctx) return SZ4_E_ARG;
  *ctx = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return SZ4_E_DEVICE;
  DeviceGuard guard(device);
  sz4_ctx* c = new sz4_ctx();
  c->device = device;
  // tuning knobs (A/B): the batch API's piece size and the stream path's chunk size in bytes
  // (sz4_set_batch_chunk / sz4_set_stream_chunk set them per context)
  if (const char* bc = getenv("SZ4_BATCH_CHUNK")) {
    const uint64_t v = strtoull(bc, nullptr, 10);
    if (v >= (1u << 20)) {
      c->batchChunk = v;
      c->batchChunkSet = true;
    }
  }
  if (const char* sc = getenv("SZ4_STREAM_CHUNK")) {
    const uint64_t v = strtoull(sc, nullptr, 10);
    if (v >= (1u << 20)) c->streamChunk = v;
  }
  // tests: allocation failures injected into the accounting, and the free memory the piece sizing assumes
  // (sz4_mem.h; sz4_debug_memory reports what they did)
  auto hook = [](const char* name) {
    const char* v = getenv(name);
    return v ? (uint64_t)strtoull(v, nullptr, 10) : 0ull;
  };
  c->budget.testAllocCap = hook("SZ4_TEST_ALLOC_CAP");
  c->budget.testFailReserve = hook("SZ4_TEST_FAIL_RESERVE");
  c->budget.testFreeBytes = hook("SZ4_TEST_FREE_BYTES");
  for (auto& e : c->ev) hipEventCreate(&e);
  for (auto& e : c->evGather) hipEventCreate(&e);
  for (auto& e : c->evMerge) hipEventCreate(&e);
  c->budget.owner = c;
  // a released plan buffer may come back at the same address: upload the plan again
  c->budget.onShed = [](void* o) { static_cast<sz4_ctx*>(o)->pipe.uploadedVersion = ~0ull; };
  if (reserve_bytes && c->pipe.staged.reserve(reserve_bytes + kPad) != hipSuccess) {
    sz4_destroy(c);
    return SZ4_E_NOMEM;
  }
  *ctx = c;
  return SZ4_OK;
}

void sz4_destroy(sz4_ctx* c)
{
  if (!c) return;
  DeviceGuard guard(c->device);
  for (DevBuf* b : c->budget.bufs) b->release();
  for (HostBuf* b : {&c->hostIn[0], &c->hostIn[1], &c->hostOut[0], &c->hostOut[1]}) b->release();
  for (hipStream_t x : {c->stream, c->upStream, c->downStream})
    if (x) hipStreamDestroy(x);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t x : {c->evUp[k], c->evDone[k]})
      if (x) hipEventDestroy(x);
  for (auto& e : c->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->evGather)
    if (e) hipEventDestroy(e);
  for (auto& e : c->evMerge)
    if (e) hipEventDestroy(e);
  delete c;
}

int sz4_acquire(sz4_ctx** ctx, int device)
{
  if (!ctx) return SZ4_E_ARG;
  static std::mutex mu;
  static std::vector<sz4_ctx*>* idle = new std::vector<sz4_ctx*>();  // never destroyed: contexts outlive exit order
  {
    std::lock_guard<std::mutex> lock(mu);
    for (size_t i = 0; i < idle->size(); i++)
      if ((*idle)[i]->device == device) {
        *ctx = (*idle)[i];
        idle->erase(idle->begin() + (long)i);
        (*ctx)->pooled = true;
        return SZ4_OK;
      }
  }
  const int r = sz4_create(ctx, device, 0);
  if (r == SZ4_OK) {
    (*ctx)->pooled = true;
    (*ctx)->poolMu = &mu;
    (*ctx)->poolIdle = idle;
  }
  return r;
}

// pooled contexts holding more device scratch than this are trimmed when they are returned
static std::atomic<uint64_t> g_poolCap{8ull << 30};

void sz4_release(sz4_ctx* c)
{
  if (!c || !c->pooled || !c->poolMu) return;
  if (c->budget.used > g_poolCap.load()) sz4_trim(c);
  std::lock_guard<std::mutex> lock(*c->poolMu);
  c->poolIdle->push_back(c);
}

void sz4_set_pool_cap(uint64_t bytes) { g_poolCap.store(bytes ? bytes : (8ull << 30)); }

void sz4_trim(sz4_ctx* c)
{
  if (!c) return;
  DeviceGuard guard(c->device);
  for (hipStream_t x : {c->stream, c->upStream, c->downStream})
    if (x) hipStreamSynchronize(x);
  for (DevBuf* b : c->budget.bufs)
    if (!b->held) b->release();  // a live decode or compress queue keeps its scratch
  for (HostBuf* b : {&c->hostIn[0], &c->hostIn[1], &c->hostOut[0], &c->hostOut[1]}) b->release();
  c->pipe.uploadedVersion = ~0ull;
}

void sz4_set_device_limit(sz4_ctx* c, uint64_t bytes)
{
  if (c) c->budget.limit = bytes;
}

uint64_t sz4_released_buffers(sz4_ctx* c) { return c ? c->budget.shedCount : 0; }

uint64_t sz4_bound(uint64_t n, uint32_t block_size)
{
  if (block_size == 0) return 0;
  const uint64_t nb = (n + block_size - 1) / block_size;
  return 16 + n + nb * 4 + 4;  // stored blocks are never larger than their input
}

uint64_t sz4_lz4_bound(uint64_t n, int legacy)
{
  const uint64_t bs = legacy ? kBlockMaxLegacy : kBlockMax;
  const uint64_t nb = n / bs + 2;
  return n + n / 255 + nb * 24 + 64;
}

int sz4_compress_blocks_device(sz4_ctx* c, const void* d_in, uint64_t n, uint32_t block_size, uint32_t max_chain,
                               int header, void* d_out, uint64_t out_cap, uint64_t* out_size, void* stream)
{
  if (!c || !out_size || (!d_in && n) || !d_out || block_size == 0 || block_size > kBlockMax || max_chain > 65535 ||
      header < SZ4_HEADER_SMALLZ4 || header > SZ4_HEADER_NONE)
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  // the kernels write the frame in place: refuse a buffer that could be overrun
  if (out_cap < sz4_bound(n, block_size)) return c->fail(SZ4_E_CAPACITY, "out_cap < sz4_bound(n, block_size)");
  DeviceGuard guard(c->device);
  try {
  hipStream_t s = (hipStream_t)stream;
  uint8_t hdr[8];
  uint64_t hl = 0;
  bool endMark = true;
  if (header == SZ4_HEADER_SMALLZ4) {
    memcpy(hdr, kFrameHeader, 7);
    hl = 7;
  } else if (header == SZ4_HEADER_INDEPENDENT) {
    uint8_t bd = 4;
    while (bd < 7 && (1ull << (8 + 2 * bd)) < block_size) bd++;
    const uint8_t desc[2] = {0x60, (uint8_t)(bd << 4)};
    const uint8_t h[7] = {0x04, 0x22, 0x4D, 0x18, desc[0], desc[1], (uint8_t)((xxh32_small(desc, 2) >> 8) & 0xFF)};
    memcpy(hdr, h, 7);
    hl = 7;
  } else {
    endMark = false;
  }
  c->batchChunked = false;
  c->pieceRetries = 0;
  c->pieceMin = ~0ull;
  if (n == 0) {
    if (out_cap < hl + (endMark ? 4 : 0)) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
    if (hl) hipMemcpyAsync(d_out, hdr, hl, hipMemcpyHostToDevice, s);
    if (endMark) hipMemsetAsync((uint8_t*)d_out + hl, 0, 4, s);
    hipStreamSynchronize(s);
    c->lastBlocks = 0;
    *out_size = hl + (endMark ? 4 : 0);
    return SZ4_OK;
  }
  // bounded memory: whole blocks in pieces of at most batchChunk input bytes, one pipeline run each
  // (the scratch is ~60-75 bytes per input byte), written one after the other into d_out
  // under a device bound the pieces shrink with it (the scratch is 36-60 bytes per piece byte)
  // Without a bound the default piece is capped so that its scratch (< kScratchPerByte per piece byte) takes at
  // most a quarter of the memory this context could use now (free + what it holds): a GPU shared with a
  // caching allocator gets smaller pieces instead of SZ4_E_NOMEM.  A piece whose reservation still fails is
  // halved and retried, down to kPieceFloor; the failed attempt's buffers are released first and
  // its error message cleared (sz4_ctx::retry_smaller)
  const uint64_t chunk = piece_bytes(c);
  // equal pieces (the last one is not a small remainder): ceil(n / chunk) of them, whole blocks each
  const uint64_t nPieces = (n + chunk - 1) / std::max<uint64_t>(chunk, 1);
  const uint64_t even = (n + nPieces - 1) / nPieces;
  uint64_t piece = std::max<uint64_t>(block_size, (even + block_size - 1) / block_size * block_size);
  float stageSum[kStages] = {};
  uint64_t pos = 0;
  c->hostBytes.clear();
  for (uint64_t off = 0; off < n; off += piece) {
    const uint64_t len = std::min(piece, n - off);
    const bool firstPiece = off == 0, lastPiece = off + len == n;
    c->pipe.plan.build_uniform(len, block_size);
    hipError_t e = hipSuccess;
    int rr = reserve_all(c, len + kPad);
    if (rr == SZ4_OK && (e = c->pipe.staged.reserve(len + kPad))) rr = c->fail(SZ4_E_NOMEM, "staging", e);
    if (rr == SZ4_E_NOMEM && piece > block_size && piece > kPieceFloor) {
      // smaller pieces: the next iteration re-plans this offset with half the piece
      piece = std::max<uint64_t>(block_size, std::max<uint64_t>(kPieceFloor, piece / 2) / block_size * block_size);
      c->retry_smaller();
      off -= piece;  // the loop adds it back (at offset 0 through the wrap)
      continue;
    }
    if (rr) return rr;
    c->pieceMin = std::min(c->pieceMin, piece);
    // private padded copy: kernels read 4-byte windows that may run past the caller's buffer
    if ((e = hipMemcpyAsync(c->pipe.staged.p, (const uint8_t*)d_in + off, len, hipMemcpyDeviceToDevice, s)))
      return c->fail(SZ4_E_DEVICE, "stage input", e);
    if ((e = hipMemsetAsync(c->pipe.staged.as<uint8_t>() + len, 0, kPad, s))) return c->fail(SZ4_E_DEVICE, "stage pad", e);
    uint64_t size = 0;
    if (int r = run_pipeline(c, RunMode{}, max_chain, c->pipe.staged.as<uint8_t>(), hdr, firstPiece ? hl : 0,
                             lastPiece && endMark, (uint8_t*)d_out + pos, out_cap - pos, &size, s))
      return r;
    pos += size;
    for (int i = 0; i < kStages; i++) stageSum[i] += c->stageMs[i];
    if (!(firstPiece && lastPiece)) {
      // every piece's block sizes, for sz4_last_block_sizes
      const uint32_t nb = (uint32_t)c->pipe.plan.blocks.size();
      const size_t at = c->hostBytes.size();
      c->hostBytes.resize(at + nb);
      if ((e = hipMemcpy(c->hostBytes.data() + at, c->pipe.blockBytes.p, nb * 4, hipMemcpyDeviceToHost)))
        return c->fail(SZ4_E_DEVICE, "block sizes", e);
    }
  }
  c->batchChunked = !c->hostBytes.empty();
  if (c->timing)
    for (int i = 0; i < kStages; i++) c->stageMs[i] = stageSum[i];
  *out_size = pos;
  return SZ4_OK;
  } catch (const std::bad_alloc&) {
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
}

int64_t sz4_last_block_sizes(sz4_ctx* c, uint32_t* sizes, uint64_t max_blocks)
{
  if (!c || !sizes) return SZ4_E_ARG;
  if (c->batchChunked) {
    const uint64_t nb = std::min<uint64_t>(c->hostBytes.size(), max_blocks);
    for (uint64_t i = 0; i < nb; i++) sizes[i] = c->hostBytes[i] & 0x7FFFFFFFu;
    return (int64_t)nb;
  }
  const uint64_t nb = std::min<uint64_t>(c->lastBlocks, max_blocks);
  if (nb * 4 > c->pipe.blockBytes.cap) return SZ4_E_DEVICE;  // released since (a failed reservation, sz4_trim)
  if (nb && hipMemcpy(sizes, c->pipe.blockBytes.p, nb * 4, hipMemcpyDeviceToHost) != hipSuccess) return SZ4_E_DEVICE;
  for (uint64_t i = 0; i < nb; i++) sizes[i] &= 0x7FFFFFFFu;
  return (int64_t)nb;
}

uint64_t sz4_batch_bound(const uint32_t* sizes, uint64_t count)
{
  uint64_t b = 0;
  for (uint64_t i = 0; sizes && i < count; i++) b += (uint64_t)sizes[i] + 4;  // stored blocks are never larger than their input
  return b;
}

// sz4_compress_batch_device (elem_sizes null), sz4_compress_batch_typed_device (filters null) and
// sz4_compress_batch_filtered_device
static int compress_batch(sz4_ctx* c, const void* const* in_ptrs, const uint32_t* in_sizes, const uint8_t* elem_sizes,
                          const uint8_t* filters, uint64_t count, uint32_t max_chain, void* d_out, uint64_t out_cap,
                          uint64_t* out_offsets, void* stream)
{
  if (!c || !out_offsets || (count && (!in_ptrs || !in_sizes)) || max_chain > 65535)
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  bool typed = false, bits = false;
  for (uint64_t i = 0; i < count; i++) {
    if (in_sizes[i] > kBlockMax) return c->fail(SZ4_E_ARG, "item larger than 4 MiB");
    if (in_sizes[i] && !in_ptrs[i]) return c->fail(SZ4_E_ARG, "null item pointer");
    if (elem_sizes) {
      const uint8_t e = elem_sizes[i];
      if (e != 1 && e != 2 && e != 4 && e != 8) return c->fail(SZ4_E_ARG, "element width is not 1, 2, 4 or 8");
      typed |= e > 1;
    }
    if (filters) {
      if (filters[i] != SZ4_FILTER_BYTES && filters[i] != SZ4_FILTER_BITS) return c->fail(SZ4_E_ARG, "unknown filter");
      bits |= filters[i] == SZ4_FILTER_BITS;
    }
  }
  if (!bits) filters = nullptr;                // the byte filter throughout: the typed call
  if (!typed && !bits) elem_sizes = nullptr;  // and widths of 1 throughout: the plain call
  // the kernels write the blocks in place: refuse a buffer that could be overrun
  const uint64_t bound = sz4_batch_bound(in_sizes, count);
  if (out_cap < bound) return c->fail(SZ4_E_CAPACITY, "out_cap < sz4_batch_bound(sizes, count)");
  if (bound && !d_out) return c->fail(SZ4_E_ARG, "bad argument");
  DeviceGuard guard(c->device);
  try {
  hipStream_t s = (hipStream_t)stream;
  // per item sizes for sz4_last_block_sizes (0 for an empty item), filled piece by piece
  c->hostBytes.assign(count, 0u);
  c->batchChunked = true;
  c->lastBlocks = 0;
  c->gatherMs = 0;
  c->pieceRetries = 0;
  c->pieceMin = ~0ull;
  float stageSum[kStages] = {};
  // bounded memory: pieces of whole items in caller order, at most `piece` staged bytes and `cap` blocks each
  // (an item larger than the piece is a piece on its own); a piece whose scratch cannot be reserved is
  // halved and tried again, down to kPieceFloor, as in sz4_compress_blocks_device
  uint64_t piece = piece_bytes(c);
  uint64_t pos = 0;
  out_offsets[0] = 0;
  for (uint64_t i = 0; i < count;) {
    const uint64_t cap = batch_block_cap(piece);
    uint64_t j = i, staged = 0, blocks = 0;
    for (; j < count; j++) {
      if (!in_sizes[j]) continue;
      const uint64_t st = batch_stride(in_sizes[j]);
      if (blocks && (staged + st > piece || blocks >= cap)) break;
      staged += st;
      blocks++;
    }
    const int r = batch_piece(c, i, j, in_ptrs, in_sizes, elem_sizes, filters, max_chain, (uint8_t*)d_out, pos,
                              c->hostBytes.data(), stageSum, s);
    if (r == SZ4_E_NOMEM && blocks > 1 && piece > kPieceFloor) {
      piece = std::max<uint64_t>(kPieceFloor, piece / 2);
      c->retry_smaller();
      continue;  // the same items again, in smaller pieces
    }
    if (r) return r;
    c->pieceMin = std::min(c->pieceMin, piece);
    for (; i < j; i++) {
      pos += c->hostBytes[i];
      out_offsets[i + 1] = pos;
    }
  }
  if (c->timing)
    for (int k = 0; k < kStages; k++) c->stageMs[k] = stageSum[k];
  return SZ4_OK;
  } catch (const std::bad_alloc&) {
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
}

int sz4_compress_batch_device(sz4_ctx* c, const void* const* in_ptrs, const uint32_t* in_sizes, uint64_t count,
                              uint32_t max_chain, void* d_out, uint64_t out_cap, uint64_t* out_offsets, void* stream)
{
  return compress_batch(c, in_ptrs, in_sizes, nullptr, nullptr, count, max_chain, d_out, out_cap, out_offsets, stream);
}

int sz4_compress_batch_typed_device(sz4_ctx* c, const void* const* in_ptrs, const uint32_t* in_sizes, const uint8_t* elem_sizes,
                                    uint64_t count, uint32_t max_chain, void* d_out, uint64_t out_cap, uint64_t* out_offsets,
                                    void* stream)
{
  if (count && !elem_sizes) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  return compress_batch(c, in_ptrs, in_sizes, elem_sizes, nullptr, count, max_chain, d_out, out_cap, out_offsets, stream);
}

int sz4_compress_batch_filtered_device(sz4_ctx* c, const void* const* in_ptrs, const uint32_t* in_sizes, const uint8_t* elem_sizes,
                                       const uint8_t* filters, uint64_t count, uint32_t max_chain, void* d_out, uint64_t out_cap,
                                       uint64_t* out_offsets, void* stream)
{
  if (count && !elem_sizes) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  return compress_batch(c, in_ptrs, in_sizes, elem_sizes, filters, count, max_chain, d_out, out_cap, out_offsets, stream);
}

float sz4_last_gather_ms(sz4_ctx* c) { return c ? c->gatherMs : 0.0f; }

float sz4_last_merge_ms(sz4_ctx* c) { return c ? c->mergeMs : 0.0f; }

// sz4_unlz4_batch_device (elem_sizes null: the blocks decode straight into d_out) and
// sz4_unlz4_batch_typed_device (they decode into unPlanes, and k_batch_merge writes d_out; filters null) and
// sz4_unlz4_batch_filtered_device (the same, with k_batch_merge_bits where an item has SZ4_FILTER_BITS)
static int unlz4_batch(sz4_ctx* c, const void* d_blocks, const uint64_t* offsets, const uint8_t* elem_sizes,
                       const uint8_t* filters, uint64_t count,
                       void* d_out, uint64_t out_cap, uint64_t* out_offsets, void* stream)
{
  if (!c || !out_offsets || (count && !offsets)) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  c->mergeMs = 0;
  bool typed = false, bits = false;
  for (uint64_t i = 0; elem_sizes && i < count; i++) {
    const uint8_t e = elem_sizes[i];
    if (e != 1 && e != 2 && e != 4 && e != 8) return c->fail(SZ4_E_ARG, "element width is not 1, 2, 4 or 8");
    typed |= e > 1;
  }
  for (uint64_t i = 0; filters && i < count; i++) {
    if (filters[i] != SZ4_FILTER_BYTES && filters[i] != SZ4_FILTER_BITS) return c->fail(SZ4_E_ARG, "unknown filter");
    bits |= filters[i] == SZ4_FILTER_BITS;
  }
  if (!bits) filters = nullptr;                // the byte filter throughout: the typed call
  if (!typed && !bits) elem_sizes = nullptr;  // and widths of 1 throughout: the plain call
  DeviceGuard guard(c->device);
  try {
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  c->unSplit = false;
  c->unIndexParallel = false;
  out_offsets[0] = 0;
  // the extents of the non-empty items; an item shorter than its size word, or longer than any LZ4 block, is corrupt
  std::vector<uint64_t> ext;
  std::vector<uint64_t> item;
  for (uint64_t i = 0; i < count; i++) {
    if (offsets[i + 1] < offsets[i]) return c->fail(SZ4_E_CORRUPT, "offsets table decreases");
    const uint64_t len = offsets[i + 1] - offsets[i];
    if (!len) continue;
    if (len < 4) return c->fail(SZ4_E_CORRUPT, "item shorter than its size word");
    if (len - 4 > kMaxFrameBlock) return c->fail(SZ4_E_CORRUPT, "item larger than any LZ4 block");
    ext.push_back(offsets[i]);
    ext.push_back(offsets[i + 1]);
    item.push_back(i);
  }
  if (item.size() >= (1ull << 31)) return c->fail(SZ4_E_ARG, "too many items");
  const uint32_t nb = (uint32_t)item.size();
  if (!nb) {
    for (uint64_t i = 0; i < count; i++) out_offsets[i + 1] = 0;
    return SZ4_OK;
  }
  if (!d_blocks) return c->fail(SZ4_E_ARG, "bad argument");
  const uint8_t* f = (const uint8_t*)d_blocks;
  const uint64_t n = offsets[count];  // every read of the passes below stays under it
  if ((e = c->unBlk.reserve(nb * sizeof(UnBlock) + 64)) || (e = c->unBatch.reserve(ext.size() * 8 + 64)) ||
      (e = c->unFlags.reserve(64)) || (e = c->unSeq.reserve(unlz4_seq_entries(n, nb) * sizeof(uint4) + 64)))
    return c->fail(SZ4_E_NOMEM, "decoder scratch", e);
  uint32_t* status = c->unFlags.as<uint32_t>();
  uint32_t st = 0;
  c->hUn.resize(nb);
  if ((e = hipMemcpyAsync(c->unBatch.p, ext.data(), ext.size() * 8, hipMemcpyHostToDevice, s)) ||
      (e = hipMemsetAsync(status, 0, 4, s)))
    return c->fail(SZ4_E_DEVICE, "decoder plan", e);
  launch_unlz4_batch_plan(f, c->unBatch.as<uint64_t>(), nb, c->unBlk.as<UnBlock>(), status, s);
  launch_unlz4_sizes(f, n, c->unBlk.as<UnBlock>(), nb, c->unSeq.as<uint4>(), s);
  if ((e = hipGetLastError()) || (e = hipMemcpyAsync(c->hUn.data(), c->unBlk.p, nb * sizeof(UnBlock), hipMemcpyDeviceToHost, s)) ||
      (e = hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
    return c->fail(SZ4_E_DEVICE, "block sizes", e);
  if (st) return c->fail(SZ4_E_CORRUPT, "size word disagrees with the item's extent");
  uint64_t w = 0;
  uint64_t i = 0;
  for (uint32_t b = 0; b < nb; b++) {
    UnBlock& B = c->hUn[b];
    if (B.size == kNone) return c->fail(SZ4_E_CORRUPT, "malformed LZ4 block");
    for (; i <= item[b]; i++) out_offsets[i] = w;
    B.dst = w;
    w += B.size;
  }
  for (; i <= count; i++) out_offsets[i] = w;
  if (w > out_cap || (w && !d_out)) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
  if (!w) return SZ4_OK;
  // typed: the blocks decode to the same offsets of a context buffer, and every item is merged on its way out
  uint8_t* target = (uint8_t*)d_out;
  std::vector<BatchTyped> merge;
  if (elem_sizes) {
    for (uint32_t b = 0; b < nb; b++)
      if (c->hUn[b].size)
        merge.push_back(BatchTyped{c->hUn[b].dst, c->hUn[b].dst, (uint32_t)c->hUn[b].size,
                                   elem_sizes[item[b]] | (bits ? (uint32_t)filters[item[b]] << kBatchFilterShift : 0u)});
    if ((e = c->unPlanes.reserve(w + 64)) || (e = c->mergeItems.reserve(merge.size() * sizeof(BatchTyped) + 64)))
      return c->fail(SZ4_E_NOMEM, "typed decoder scratch", e);
    target = c->unPlanes.as<uint8_t>();
    if ((e = hipMemcpyAsync(c->mergeItems.p, merge.data(), merge.size() * sizeof(BatchTyped), hipMemcpyHostToDevice, s)))
      return c->fail(SZ4_E_DEVICE, "upload items", e);
  }
  if ((e = hipMemcpyAsync(c->unBlk.p, c->hUn.data(), nb * sizeof(UnBlock), hipMemcpyHostToDevice, s)) ||
      (e = hipMemsetAsync(status, 0, 4, s)))
    return c->fail(SZ4_E_DEVICE, "decoder plan", e);
  launch_unlz4_blocks_indep(f, n, c->unBlk.as<UnBlock>(), nb, c->unSeq.as<uint4>(), target, status, s);
  if (elem_sizes) {
    if (c->timing) hipEventRecord(c->evMerge[0], s);
    if (bits) launch_batch_merge_bits(c->mergeItems.as<BatchTyped>(), (uint32_t)merge.size(), target, (uint8_t*)d_out, w, s);
    else launch_batch_merge(c->mergeItems.as<BatchTyped>(), (uint32_t)merge.size(), target, (uint8_t*)d_out, w, s);
    if (c->timing) hipEventRecord(c->evMerge[1], s);
  }
  if ((e = hipGetLastError()) || (e = hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, s)) ||
      (e = hipStreamSynchronize(s)))
    return c->fail(SZ4_E_DEVICE, "decode", e);
  if (st) return c->fail(SZ4_E_DEVICE, "decoded length differs from the size pass");
  if (elem_sizes && c->timing && hipEventElapsedTime(&c->mergeMs, c->evMerge[0], c->evMerge[1]) != hipSuccess) c->mergeMs = 0;
  return SZ4_OK;
  } catch (const std::bad_alloc&) {
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
}

int sz4_unlz4_batch_device(sz4_ctx* c, const void* d_blocks, const uint64_t* offsets, uint64_t count, void* d_out,
                           uint64_t out_cap, uint64_t* out_offsets, void* stream)
{
  return unlz4_batch(c, d_blocks, offsets, nullptr, nullptr, count, d_out, out_cap, out_offsets, stream);
}

int sz4_unlz4_batch_typed_device(sz4_ctx* c, const void* d_blocks, const uint64_t* offsets, const uint8_t* elem_sizes,
                                 uint64_t count, void* d_out, uint64_t out_cap, uint64_t* out_offsets, void* stream)
{
  if (count && !elem_sizes) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  return unlz4_batch(c, d_blocks, offsets, elem_sizes, nullptr, count, d_out, out_cap, out_offsets, stream);
}

int sz4_unlz4_batch_filtered_device(sz4_ctx* c, const void* d_blocks, const uint64_t* offsets, const uint8_t* elem_sizes,
                                    const uint8_t* filters, uint64_t count, void* d_out, uint64_t out_cap, uint64_t* out_offsets,
                                    void* stream)
{
  if (count && !elem_sizes) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  return unlz4_batch(c, d_blocks, offsets, elem_sizes, filters, count, d_out, out_cap, out_offsets, stream);
}

// ---- decode queue: everything an enqueue needs, reserved once on the context's budget and held -----------
static_assert(SZ4_ITEM_OK == kItemOk && SZ4_ITEM_CORRUPT == kItemCorrupt && SZ4_ITEM_CAPACITY == kItemCapacity &&
                  SZ4_ITEM_ARG == kItemArg && SZ4_ITEM_QUEUE == kItemQueue && SZ4_ITEM_INTERNAL == kItemInternal,
              "the kernels' item statuses are the header's");

struct sz4_dq {
  sz4_ctx* ctx;
  uint32_t maxItems;
  uint64_t maxSrc;
  DevBuf blk, seqOff, seq;  // UnBlock and list offset per item; the sequence lists
  sz4_dq(sz4_ctx* c, uint32_t items, uint64_t src)
      : ctx(c), maxItems(items), maxSrc(src), blk(c->budget, true), seqOff(c->budget, true), seq(c->budget, true) {}
  void detach()
  {
    for (DevBuf* b : {&blk, &seqOff, &seq}) b->detach();
  }
};

int sz4_dq_create(sz4_ctx* c, uint32_t max_items, uint64_t max_src_bytes, sz4_dq** q)
{
  if (q) *q = nullptr;
  if (!c || !q) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  if (max_items < 1 || max_items > 65536) return c->fail(SZ4_E_ARG, "max_items is not 1 .. 65536");
  c->begin_call();
  DeviceGuard guard(c->device);
  sz4_dq* d = new (std::nothrow) sz4_dq(c, max_items, max_src_bytes);
  if (!d) return c->fail(SZ4_E_NOMEM, "host allocation");
  hipError_t e;
  if ((e = d->blk.reserve((uint64_t)max_items * sizeof(UnBlock))) || (e = d->seqOff.reserve((uint64_t)max_items * 8)) ||
      (e = d->seq.reserve(unlz4_seq_entries(max_src_bytes, max_items) * sizeof(uint4)))) {
    d->detach();
    delete d;
    return c->fail(SZ4_E_NOMEM, "decode queue scratch", e);
  }
  *q = d;
  return SZ4_OK;
}

void sz4_dq_destroy(sz4_dq* q)
{
  if (!q) return;
  DeviceGuard guard(q->ctx->device);
  q->detach();
  delete q;
}

// Launches only: no allocation, no copy, no wait, and nothing of the context's call state is touched
int sz4_dq_enqueue(sz4_dq* q, const void* const* d_src, const uint32_t* d_src_sizes, void* const* d_dst,
                   const uint32_t* d_dst_caps, const uint8_t* d_elems, uint32_t count, uint32_t* d_out_sizes,
                   uint32_t* d_status, void* stream)
{
  if (!q || !d_src || !d_src_sizes || !d_dst || !d_dst_caps || !d_out_sizes || !d_status || count > q->maxItems)
    return SZ4_E_ARG;
  if (!count) return SZ4_OK;
  DeviceGuard guard(q->ctx->device);
  const DqTables T{reinterpret_cast<const uint64_t*>(d_src), d_src_sizes, reinterpret_cast<const uint64_t*>(d_dst),
                   d_dst_caps, d_elems, d_out_sizes, d_status};
  launch_unlz4_dq(T, count, q->maxSrc, q->blk.as<UnBlock>(), q->seqOff.as<uint64_t>(), q->seq.as<uint4>(),
                  (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SZ4_OK : SZ4_E_DEVICE;
}

// ---- compress queue: a ragged run planned, reserved and uploaded once, in a pipe of its own (held) ------------
struct sz4_cq {
  sz4_ctx* ctx;
  uint32_t count = 0;        // caller items
  uint32_t maxChain = 0;
  bool planes = false;       // an item is wider than 1: the item table is BatchTyped, staged by k_batch_gather_planes
  bool sized = false;        // sz4_cq_create_sized: the sizes are capacities, every item has a slot (block i is item i)
  uint64_t bound = 0;        // sz4_batch_bound of the sizes
  uint64_t stagedBytes = 0;  // the gather's extent: the items' strides and the pad
  uint64_t longBitsBytes = 0;
  Pipe pipe;
  DevBuf map;                // per caller item: its block (CqTables::map); a sized queue has none
  DevBuf slots;              // a sized queue's Slot table (sz4_slot_plan.h), read by k_cq_plan
  PipeArgs args{};           // the launchers' view of `pipe`, but for the output address
  explicit sz4_cq(sz4_ctx* c) : ctx(c), pipe(c->budget, true), map(c->budget, true), slots(c->budget, true) {}
  void detach()
  {
    pipe.detach();
    map.detach();
    slots.detach();
  }
};

// both kinds of queue: `sizes` are the items' sizes, or (sized) their capacities
static int cq_create(sz4_ctx* c, const uint32_t* sizes, const uint8_t* elem_sizes, uint32_t count, uint32_t max_chain,
                     bool sized, sz4_cq** q)
{
  if (q) *q = nullptr;
  if (!c || !q || (count && !sizes)) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  if (count < 1 || count > kBatchMaxBlocks) return c->fail(SZ4_E_ARG, "count is not 1 .. 32768");
  if ((max_chain >= 1 && max_chain <= (uint32_t)kLazyMax) || max_chain > 65535)
    return c->fail(SZ4_E_ARG, "a compress queue runs level 0 and max_chain 7 .. 65535 (levels 1 .. 6 read status words on the host)");
  uint64_t staged = 0;
  bool planes = false;
  for (uint32_t i = 0; i < count; i++) {
    if (sizes[i] > kBlockMax) return c->fail(SZ4_E_ARG, "item larger than 4 MiB");
    const uint8_t e = elem_sizes ? elem_sizes[i] : 1;
    if (e != 1 && e != 2 && e != 4 && e != 8) return c->fail(SZ4_E_ARG, "element width is not 1, 2, 4 or 8");
    planes |= e > 1;
    staged += batch_stride(sizes[i]);
  }
  if (staged > kBatchChunkDefault) return c->fail(SZ4_E_ARG, "the items stage more than 448 MiB");
  c->begin_call();
  DeviceGuard guard(c->device);
  sz4_cq* d = nullptr;
  try {
    d = new sz4_cq(c);
    d->count = count;
    d->maxChain = max_chain;
    d->planes = planes;
    d->sized = sized;
    d->bound = sz4_batch_bound(sizes, count);
    // the non-empty items are the plan's blocks, in caller order; an empty item maps to the block that follows it
    // (a sized queue: every item is a block, in its slot, whatever its capacity)
    std::vector<uint64_t> runSizes;
    std::vector<uint32_t> map(count);
    for (uint32_t i = 0; i < count; i++) {
      map[i] = sized ? i : (uint32_t)runSizes.size() | (sizes[i] ? 0u : kCqEmpty);
      if (sizes[i] && !sized) runSizes.push_back(sizes[i]);
    }
    const uint32_t nb = sized ? count : (uint32_t)runSizes.size();
    Pipe& P = d->pipe;
    if (sized) {
      d->stagedBytes = P.plan.build_slots(std::vector<uint32_t>(sizes, sizes + count)) + kPad;
      for (uint32_t i = 0; i < count; i++) P.plan.slots[i].elem = elem_sizes ? elem_sizes[i] : 1;
    } else {
      d->stagedBytes = P.plan.build_ragged(runSizes) + kPad;
    }
    d->longBitsBytes = nb ? P.plan.blocks.back().end / 8 + 8 : 0;
    // the item table with everything but the sources, which k_cq_items fills in on every enqueue
    std::vector<BatchItem> items(planes ? 0 : nb);
    std::vector<BatchTyped> typed(planes ? nb : 0);
    for (uint32_t i = 0; i < count; i++) {
      if (!sizes[i] && !sized) continue;
      const uint32_t b = map[i];
      if (planes) typed[b] = BatchTyped{0, P.plan.blocks[b].start, sizes[i], elem_sizes[i]};
      else items[b] = BatchItem{0, P.plan.blocks[b].start, sizes[i]};
    }
    hipError_t e;
    if ((e = P.reserve(d->stagedBytes)) || (e = P.staged.reserve(d->stagedBytes)) ||
        (e = P.batchItems.reserve(nb * sizeof(BatchItem) + 64)) || (!sized && (e = d->map.reserve(count * 4ull))) ||
        (sized && (e = d->slots.reserve(count * sizeof(Slot))))) {
      d->detach();
      delete d;
      return c->fail(SZ4_E_NOMEM, "compress queue scratch", e);
    }
    if ((e = P.upload_plan(nullptr)) ||
        (nb && (e = hipMemcpyAsync(P.batchItems.p, planes ? (const void*)typed.data() : (const void*)items.data(),
                                   nb * sizeof(BatchItem), hipMemcpyHostToDevice, nullptr))) ||
        (!sized && (e = hipMemcpyAsync(d->map.p, map.data(), count * 4ull, hipMemcpyHostToDevice, nullptr))) ||
        (sized && (e = hipMemcpyAsync(d->slots.p, P.plan.slots.data(), count * sizeof(Slot), hipMemcpyHostToDevice, nullptr))) ||
        (e = hipStreamSynchronize(nullptr))) {
      d->detach();
      delete d;
      return c->fail(SZ4_E_DEVICE, "upload plan", e);
    }
    d->args = P.args(max_chain, P.staged.as<uint8_t>(), nullptr, 0);
  } catch (const std::bad_alloc&) {
    if (d) {
      d->detach();
      delete d;
    }
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
  *q = d;
  return SZ4_OK;
}

int sz4_cq_create(sz4_ctx* c, const uint32_t* sizes, const uint8_t* elem_sizes, uint32_t count, uint32_t max_chain, sz4_cq** q)
{
  return cq_create(c, sizes, elem_sizes, count, max_chain, false, q);
}

int sz4_cq_create_sized(sz4_ctx* c, const uint32_t* caps, const uint8_t* elem_sizes, uint32_t count, uint32_t max_chain,
                        sz4_cq** q)
{
  return cq_create(c, caps, elem_sizes, count, max_chain, true, q);
}

void sz4_cq_destroy(sz4_cq* q)
{
  if (!q) return;
  DeviceGuard guard(q->ctx->device);
  q->detach();
  delete q;
}

uint64_t sz4_cq_bound(const sz4_cq* q) { return q ? q->bound : 0; }

// Kernel launches only: no allocation, no copy, no wait, and nothing of the context's call state is touched.
// The launch sequence is run_pipeline's for independent blocks at level 0 and the parsed levels, where it reads
// nothing back; what run_pipeline clears with memsets (and the ghost slot it uploads) k_cq_items and k_cq_zero
// clear, because a captured memset did not replay reliably.  A sized queue (d_src_sizes) starts with k_cq_plan
// in k_cq_items' place; the grids that follow are the capacity plan's, whatever the sizes
static int cq_enqueue(sz4_cq* q, const void* const* d_src, const uint32_t* d_src_sizes, void* d_out, uint64_t out_cap,
                      uint64_t* d_block_ptrs, uint32_t* d_block_sizes, uint32_t* d_status, uint64_t* d_total, void* stream)
{
  if (!q || !d_src || !d_out || !d_block_ptrs || !d_block_sizes || !d_status || q->sized != (d_src_sizes != nullptr))
    return SZ4_E_ARG;
  if (out_cap < q->bound) return SZ4_E_CAPACITY;
  DeviceGuard guard(q->ctx->device);
  hipStream_t s = (hipStream_t)stream;
  PipeArgs P = q->args;
  P.out = (uint8_t*)d_out;
  const uint32_t nb = P.nblocks;
  const CqTables T{reinterpret_cast<const uint64_t*>(d_src), q->sized ? nullptr : q->map.as<uint32_t>(), q->count, P.out,
                   d_block_ptrs, d_block_sizes, d_status, d_total};
  if (q->sized) launch_cq_plan(T, d_src_sizes, q->slots.as<Slot>(), P, q->pipe.batchItems.p, q->planes, s);
  else launch_cq_items(T, P, q->pipe.batchItems.p, q->planes, s);
  if (nb) {
    uint8_t* staged = q->pipe.staged.as<uint8_t>();
    if (q->planes) launch_batch_gather_planes(q->pipe.batchItems.as<BatchTyped>(), nb, staged, q->stagedBytes, s);
    else launch_batch_gather(q->pipe.batchItems.as<BatchItem>(), nb, staged, q->stagedBytes, s);
    launch_runs(P, s);
    if (q->maxChain > 0) {
      launch_cq_zero(P.longBits, q->longBitsBytes, s);
      launch_find(1, P, s);
      launch_find(2, P, s);
    }
    launch_prep(P, s);
    launch_parse(P, s);
    launch_emit(P, s);
  }
  launch_cq_finish(T, P, s);
  return hipGetLastError() == hipSuccess ? SZ4_OK : SZ4_E_DEVICE;
}

int sz4_cq_enqueue(sz4_cq* q, const void* const* d_src, void* d_out, uint64_t out_cap, uint64_t* d_block_ptrs,
                   uint32_t* d_block_sizes, uint32_t* d_status, uint64_t* d_total, void* stream)
{
  return cq_enqueue(q, d_src, nullptr, d_out, out_cap, d_block_ptrs, d_block_sizes, d_status, d_total, stream);
}

int sz4_cq_enqueue_sized(sz4_cq* q, const void* const* d_src, const uint32_t* d_src_sizes, void* d_out, uint64_t out_cap,
                         uint64_t* d_block_ptrs, uint32_t* d_block_sizes, uint32_t* d_status, uint64_t* d_total,
                         void* stream)
{
  if (!d_src_sizes) return SZ4_E_ARG;  // (cq_enqueue would take it for the fixed queue's call)
  return cq_enqueue(q, d_src, d_src_sizes, d_out, out_cap, d_block_ptrs, d_block_sizes, d_status, d_total, stream);
}

int sz4_lz4_stream(sz4_ctx* c, sz4_get_bytes get_bytes, sz4_send_bytes send_bytes, uint32_t max_chain, const void* dict,
                   uint64_t dict_len, int legacy, void* user)
{
  if (!c || !get_bytes || !send_bytes || max_chain > 65535 || (dict_len && !dict))
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  DeviceGuard guard(c->device);
  return stream_compress(c, get_bytes, send_bytes, max_chain, (const uint8_t*)dict, dict_len, legacy, user);
}

int sz4_lz4(sz4_ctx* c, const void* in, uint64_t n, uint32_t max_chain, const void* dict, uint64_t dict_len, int legacy,
            void* out, uint64_t out_cap, uint64_t* out_size)
{
  if (!c || !out_size || (!in && n) || !out || max_chain > 65535 || (dict_len && !dict))
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  DeviceGuard guard(c->device);
  // the stream path over memory: the source hands out 64 KiB pieces, the sink appends
  MemSource src{(const uint8_t*)in, n, 0};
  MemSink dst{(uint8_t*)out, out_cap, 0};
  const int r = stream_compress(c, mem_get, mem_send, max_chain, (const uint8_t*)dict, dict_len, legacy, &src, &dst);
  if (r != SZ4_OK) return r;
  if (dst.n > out_cap) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
  *out_size = dst.n;
  return SZ4_OK;
}

void sz4_set_stream_chunk(sz4_ctx* c, uint64_t bytes)
{
  if (c) c->streamChunk = bytes ? bytes : (64ull << 20);
}

void sz4_set_batch_chunk(sz4_ctx* c, uint64_t bytes)
{
  if (c) {
    c->batchChunk = bytes ? bytes : kBatchChunkDefault;
    c->batchChunkSet = bytes != 0;
  }
}

int sz4_last_stage_ms(sz4_ctx* c, float* stage_ms, int n)
{
  if (!c || !stage_ms) return SZ4_E_ARG;
  const int k = std::min(n, kStages);
  for (int i = 0; i < k; i++) stage_ms[i] = c->stageMs[i];
  return kStages;
}

void sz4_set_timing(sz4_ctx* c, int on)
{
  if (c) c->timing = on != 0;
}

void sz4_debug_stop_after(sz4_ctx* c, int stop_after)
{
  if (c) c->stopAfter = stop_after;
}

int sz4_debug_memory(sz4_ctx* c, uint64_t out[4])
{
  if (!c || !out) return SZ4_E_ARG;
  out[0] = c->budget.growths;
  out[1] = c->budget.injected;
  out[2] = c->pieceRetries;
  out[3] = c->pieceMin == ~0ull ? 0 : c->pieceMin;
  return SZ4_OK;
}

static int debug_copy(sz4_ctx* c, bool choices, uint32_t* len, uint16_t* dist, uint64_t n)
{
  if (!c || !len || !dist) return SZ4_E_ARG;
  if (n * 4 > c->pipe.mlen.cap || n * 2 > c->pipe.mdist.cap) return SZ4_E_ARG;
  const uint32_t* lens = choices ? c->pipe.sel() : c->pipe.mlen.as<uint32_t>();
  if (hipMemcpy(len, lens, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(dist, c->pipe.mdist.p, n * 2, hipMemcpyDeviceToHost) != hipSuccess)
    return SZ4_E_DEVICE;
  return SZ4_OK;
}

int sz4_debug_matches(sz4_ctx* c, uint32_t* len, uint16_t* dist, uint64_t n)
{
  // after the parse at optimal levels the lengths are the parse's choices
  return debug_copy(c, c && c->stopAfter == 4 && c->lastChain > (uint32_t)kGreedyMax, len, dist, n);
}

int sz4_debug_parse_input(sz4_ctx* c, uint32_t* len, uint16_t* dist, uint64_t n)
{
  return debug_copy(c, false, len, dist, n);
}

int sz4_unlz4_device(sz4_ctx* c, const void* d_frame, uint64_t frame_len, const void* d_dict, uint64_t dict_len,
                     void* d_out, uint64_t out_cap, uint64_t* out_size, void* stream)
{
  if (!c || !out_size || (!d_frame && frame_len) || (dict_len && !d_dict))
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  DeviceGuard guard(c->device);
  hipStream_t s = (hipStream_t)stream;
  uint64_t total = 0;
  uint32_t keep = 0;
  if (int r = unlz4_plan(c, (const uint8_t*)d_frame, frame_len, &total, &keep, s)) return r;
  *out_size = total;
  if (total > out_cap || (total && !d_out)) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
  // the dictionary's last 64 KiB precede the output (smallz4cat.c:168-187)
  const uint64_t dl = std::min<uint64_t>(dict_len, 65536);
  const uint8_t* dict = dl ? (const uint8_t*)d_dict + (dict_len - dl) : nullptr;
  return unlz4_decode(c, (const uint8_t*)d_frame, frame_len, dict, dl, (uint8_t*)d_out, keep, s);
}

int sz4_unlz4(sz4_ctx* c, const void* frame, uint64_t frame_len, const void* dict, uint64_t dict_len, void* out,
              uint64_t out_cap, uint64_t* out_size)
{
  if (!c || !out_size || (!frame && frame_len) || (dict_len && !dict))
    return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  DeviceGuard guard(c->device);
  hipError_t e;
  const uint64_t dl = std::min<uint64_t>(dict_len, 65536);
  if ((e = c->unFrame.reserve(frame_len + 64)) || (e = c->unDict.reserve(dl + 64)))
    return c->fail(SZ4_E_NOMEM, "staging", e);
  if ((frame_len && (e = hipMemcpy(c->unFrame.p, frame, frame_len, hipMemcpyHostToDevice))) ||
      (dl && (e = hipMemcpy(c->unDict.p, (const uint8_t*)dict + (dict_len - dl), dl, hipMemcpyHostToDevice))))
    return c->fail(SZ4_E_DEVICE, "upload", e);
  uint64_t total = 0;
  uint32_t keep = 0;
  if (int r = unlz4_plan(c, c->unFrame.as<uint8_t>(), frame_len, &total, &keep, nullptr)) return r;
  *out_size = total;
  if (total > out_cap || (total && !out)) return c->fail(SZ4_E_CAPACITY, "output buffer too small");
  if (!total) return SZ4_OK;
  if (int r = unlz4_reserve_out(c, c->unFrame.as<uint8_t>(), frame_len, &total, &keep)) return r;
  if (int r = unlz4_decode(c, c->unFrame.as<uint8_t>(), frame_len, dl ? c->unDict.as<uint8_t>() : nullptr, dl,
                           c->unOut.as<uint8_t>(), keep, nullptr))
    return r;
  if ((e = hipMemcpy(out, c->unOut.p, total, hipMemcpyDeviceToHost))) return c->fail(SZ4_E_DEVICE, "download", e);
  return SZ4_OK;
}

int sz4_unlz4_stream(sz4_ctx* c, sz4_get_byte get_byte, sz4_send_out send_bytes, const void* dict, uint64_t dict_len,
                     void* user)
{
  if (!c || !get_byte || !send_bytes || (dict_len && !dict)) return c ? c->fail(SZ4_E_ARG, "bad argument") : SZ4_E_ARG;
  c->begin_call();
  DeviceGuard guard(c->device);
  try {
    return stream_decompress(c, get_byte, send_bytes, (const uint8_t*)dict, dict_len, user);
  } catch (const std::bad_alloc&) {
    return c->fail(SZ4_E_NOMEM, "host allocation");
  }
}

uint64_t sz4_device_bytes(sz4_ctx* c)
{
  if (!c) return 0;
  return c->budget.used;
}

uint32_t sz4_dict_rounds(sz4_ctx* c) { return c ? c->dictRounds : 0u; }

uint32_t sz4_unlz4_resolve_passes(sz4_ctx* c) { return c && c->unSplit ? c->unResolvePasses : 0u; }

int sz4_unlz4_index_parallel(sz4_ctx* c) { return c && c->unIndexParallel ? 1 : 0; }

const char* sz4_last_error(sz4_ctx* c) { return c ? c->err.c_str() : "no context"; }

}  // extern "C"
