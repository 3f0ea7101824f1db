// snapshot_kernel.h — the mailbox kernels of snapshot / restore / fork.
//
// rec, the mailbox region, is rec_per_block = D*N*NS*M*64 records of 16 B per 64-cluster block and
// almost all of it is dead: a bucket's live records are the first cnt[box][lane] of its M, and
// nothing ever reads past them (the compaction swap moves only those, init never clears rec).  A
// snapshot therefore carries the live records alone, packed by these kernels; the counts travel
// with the tile image and say where each record belongs, so the stream holds no masks.
//
// One wave per 64-cluster block, indexed by slot (slot_of / cl_of travel in the arena, so the
// compaction's permutation comes along as it is).  The walk is the same in all four kernels: boxes
// in index order, in a box positions k = 0, 1, ... while any lane has k < cnt, in a position the
// lanes with k < cnt in lane order.  Reads of rec are the layout's natural 1-KB rows
// ([box][k][lane] x 16 B), writes to the stream are contiguous.  Blocks past the live bound and
// frozen clusters have zero counts and cost their count rows only.  Counts are clamped to M, so a
// wrong count cannot take an index out of its box.
#pragma once
#include "paxisim_dev.h"

namespace pxs {

constexpr uint32_t SNAP_WAVES = 4;   // waves (blocks) per workgroup

__device__ __forceinline__ const uint8_t* mbox_cnt_of(const uint8_t* image, const Image& img, uint64_t blk) {
  return image + (size_t)blk * img.bytes + img.off_cnt;
}

// Live records of each block: the sum of its u8 counts over the D*N*NS boxes and 64 lanes.  The
// count rows of a block are nbox*64 contiguous bytes (4-byte aligned), read a word per lane.
__global__ void mbox_count(const uint8_t* image, Image img, uint32_t nbox, uint32_t M, uint64_t blocks,
                           unsigned long long* per_block) {
  const uint64_t blk = (uint64_t)blockIdx.x * SNAP_WAVES + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (blk >= blocks) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(mbox_cnt_of(image, img, blk));
  uint32_t n = 0;
  for (uint32_t i = lane; i < nbox * (LANES / 4u); i += LANES) {
    const uint32_t v = w[i];
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t c = (v >> (8u * b)) & 0xFFu;
      n += c < M ? c : M;
    }
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
  if (lane == 0) per_block[blk] = n;
}

// Exclusive scan of the block totals in place (one workgroup of 1024); the grand total to *total.
__global__ void mbox_scan(unsigned long long* per_block, uint64_t blocks, unsigned long long* total) {
  __shared__ unsigned long long sh[1024];
  __shared__ unsigned long long carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < blocks; base += 1024) {
    const unsigned long long v = base + tid < blocks ? per_block[base + tid] : 0ull;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
      const unsigned long long t = tid >= off ? sh[tid - off] : 0ull;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (base + tid < blocks) per_block[base + tid] = carry + sh[tid] - v;
    __syncthreads();
    if (tid == 0) carry += sh[1023];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// The walk over one block's live records: f(index in the block's rec, position in the block's run
// of the stream) for every live record of this lane; returns the block's record count.
template <class F>
__device__ __forceinline__ uint64_t mbox_walk(const uint8_t* cnt, uint32_t nbox, uint32_t M, uint32_t lane, F f) {
  uint64_t off = 0;   // wave-uniform
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t b = 0; b < nbox; b++) {
    uint32_t c = cnt[(b << 6) | lane];
    c = c < M ? c : M;
    for (uint32_t k = 0;; k++) {
      const uint64_t mask = __ballot(k < c);
      if (!mask) break;
      if (k < c) f(((size_t)(b * M + k) << 6) | lane, off + (uint64_t)__popcll(mask & below));
      off += (uint64_t)__popcll(mask);
    }
  }
  return off;
}

// rec -> the packed stream; offs: the scanned block totals, total: the stream's length in records
__global__ void mbox_pack(const uint8_t* image, Image img, const uint4* rec, uint32_t rec_per_block, uint32_t nbox,
                          uint32_t M, uint64_t blocks, const unsigned long long* offs, uint64_t total, uint4* out) {
  const uint64_t blk = (uint64_t)blockIdx.x * SNAP_WAVES + (threadIdx.x >> 6);
  if (blk >= blocks) return;
  const uint4* r = rec + (size_t)blk * rec_per_block;
  const uint64_t o0 = offs[blk];
  mbox_walk(mbox_cnt_of(image, img, blk), nbox, M, threadIdx.x & 63u, [&](size_t i, uint64_t o) {
    if (o0 + o < total) out[o0 + o] = r[i];
  });
}

// The mirror, run once the image section (with the counts) is in place.  Dead slots of rec are
// left as they are: whatever they hold is never read.
__global__ void mbox_unpack(const uint8_t* image, Image img, uint4* rec, uint32_t rec_per_block, uint32_t nbox,
                            uint32_t M, uint64_t blocks, const unsigned long long* offs, uint64_t total, const uint4* in) {
  const uint64_t blk = (uint64_t)blockIdx.x * SNAP_WAVES + (threadIdx.x >> 6);
  if (blk >= blocks) return;
  uint4* r = rec + (size_t)blk * rec_per_block;
  const uint64_t o0 = offs[blk];
  mbox_walk(mbox_cnt_of(image, img, blk), nbox, M, threadIdx.x & 63u, [&](size_t i, uint64_t o) {
    if (o0 + o < total) r[i] = in[o0 + o];
  });
}

// fork: the same walk from one handle's rec into another's of the same plan, no packed stage
__global__ void mbox_copy_live(const uint8_t* image, Image img, const uint4* src, uint4* dst, uint32_t rec_per_block,
                               uint32_t nbox, uint32_t M, uint64_t blocks) {
  const uint64_t blk = (uint64_t)blockIdx.x * SNAP_WAVES + (threadIdx.x >> 6);
  if (blk >= blocks) return;
  const uint4* s = src + (size_t)blk * rec_per_block;
  uint4* d = dst + (size_t)blk * rec_per_block;
  mbox_walk(mbox_cnt_of(image, img, blk), nbox, M, threadIdx.x & 63u, [&](size_t i, uint64_t) { d[i] = s[i]; });
}

}  // namespace pxs
