// flowsim_snap.h -- snapshots of a handle (include/flowsim.h fs_snapshot_*): the table of everything a kernel or an fs_*
// call writes after fs_create (built once by Sim<T>::build_snapshot_table, flowsim_sim.h) and the ONE kernel that moves all
// of it, handle -> blob or blob -> handle, for the replicas a mask selects.
//
// The blob is field after field, each [R][row bytes] exactly as the handle holds it, every field starting at a multiple
// of 16 bytes.  A replica's row of a field is therefore at the same offset from the field's start on both sides, and a
// group of SNAP_GROUP = 8 consecutive replicas starts 16-byte aligned on both sides whenever the field does (every row
// is a whole number of 2-byte words: 8 rows are a whole number of 16-byte words).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fs {

enum { SNAP_MAX_FIELDS = 48, SNAP_GROUP = 8 };

// the field tags (part of the layout fingerprint: never renumber, append)
enum SnapTag {
  SNAP_POS = 1, SNAP_VEL, SNAP_PREV_VEL, SNAP_ACCEL, SNAP_CTRL_STATE, SNAP_LANE, SNAP_LAST_LC, SNAP_TIME, SNAP_SORT_KEY,
  SNAP_NOISE_CTR, SNAP_RING_LEN, SNAP_INIT_RING_LEN, SNAP_ST16_HI, SNAP_ST16_LO, SNAP_ST16_VEL, SNAP_PIS_HIST, SNAP_PIS_N,
  SNAP_INIT_POS, SNAP_INIT_VEL, SNAP_INIT_LANE, SNAP_SEQ, SNAP_ORIGIN, SNAP_FOLL, SNAP_FOLL_H, SNAP_CTL_SEQ, SNAP_LEAD,
  SNAP_HEADWAY, SNAP_VMAX, SNAP_ARRIVED_RL, SNAP_ARR_HIST, SNAP_COUNTERS, SNAP_EMITTED, SNAP_GENERATED, SNAP_FLOW_PER,
  SNAP_INIT_FLOW_PER, SNAP_EPISODE, SNAP_POL_CTR, SNAP_OBS
};

struct SnapEntry {
  char* ptr;                 // the handle's array [R][row]
  unsigned long long off;    // the field's start in the blob (a multiple of 16)
  unsigned row;              // bytes per replica
  unsigned tag;              // SnapTag
};

struct SnapTable {           // a kernel argument: read with scalar loads, indexed by the (wave-uniform) field
  SnapEntry e[SNAP_MAX_FIELDS];
  int n;
  int R;
};

// n bytes, by the whole wave: 16-byte accesses where both addresses are 16-byte aligned, then 4-byte ones where both are
// 4-byte aligned, then bytes (the tail of a row of halves).  dst, src and n are wave-uniform.
__device__ __forceinline__ void snap_copy(char* __restrict__ dst, const char* __restrict__ src, size_t n, int lane) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
  size_t at = 0;
  if ((a & 15) == 0) {
    const size_t n16 = n >> 4;
    for (size_t i = lane; i < n16; i += 64) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    at = n16 << 4;
  }
  if ((a & 3) == 0) {
    const size_t n4 = (n - at) >> 2;
    for (size_t i = lane; i < n4; i += 64)
      reinterpret_cast<uint32_t*>(dst + at)[i] = reinterpret_cast<const uint32_t*>(src + at)[i];
    at += n4 << 2;
  }
  for (size_t i = at + lane; i < n; i += 64) dst[i] = src[i];
}

// One wave per (field, group of 8 replicas), grid-strided; consecutive waves take consecutive groups of one field.  A wave
// whose replicas are all unselected goes on without touching either side; one whose replicas are all selected copies their
// rows as one span; a mixed one copies the selected rows one by one.  No LDS, no scratch, no atomics.
template <bool RESTORE>
__global__ __launch_bounds__(256) void k_snapshot(SnapTable t, char* __restrict__ blob, const uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int((blockIdx.x * 256u + threadIdx.x) >> 6));
  const int nwaves = int(gridDim.x) * 4;
  const int groups = (t.R + SNAP_GROUP - 1) / SNAP_GROUP;
  const long long items = (long long)groups * t.n;
  for (long long w = wave; w < items; w += nwaves) {
    const int f = int(w / groups), g = int(w - (long long)f * groups);
    const int r0 = g * SNAP_GROUP;
    const int nr = t.R - r0 < SNAP_GROUP ? t.R - r0 : SNAP_GROUP;
    const unsigned all = (1u << nr) - 1u;
    unsigned sel = all;
    if (mask != nullptr) {
      sel = 0u;
      for (int j = 0; j < nr; ++j) sel |= (mask[r0 + j] != 0 ? 1u : 0u) << j;
    }
    if (sel == 0u) continue;
    const SnapEntry en = t.e[f];
    char* hp = en.ptr + size_t(r0) * en.row;
    char* bp = blob + en.off + size_t(r0) * en.row;
    if (sel == all) {
      if (RESTORE) snap_copy(hp, bp, size_t(nr) * en.row, lane);
      else snap_copy(bp, hp, size_t(nr) * en.row, lane);
      continue;
    }
    for (int j = 0; j < nr; ++j) {
      if (!((sel >> j) & 1u)) continue;
      if (RESTORE) snap_copy(hp + size_t(j) * en.row, bp + size_t(j) * en.row, en.row, lane);
      else snap_copy(bp + size_t(j) * en.row, hp + size_t(j) * en.row, en.row, lane);
    }
  }
}

// (the caller has checked the blob's size against the table: fs_snapshot_info.bytes)
inline hipError_t launch_snapshot(hipStream_t stream, const SnapTable& t, bool restore, char* blob, const uint8_t* mask) {
  const long long groups = (t.R + SNAP_GROUP - 1) / SNAP_GROUP;
  const long long items = groups * t.n;
  long long blocks = (items + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  if (restore) hipLaunchKernelGGL((k_snapshot<true>), dim3(unsigned(blocks)), dim3(256), 0, stream, t, blob, mask);
  else hipLaunchKernelGGL((k_snapshot<false>), dim3(unsigned(blocks)), dim3(256), 0, stream, t, blob, mask);
  return hipGetLastError();
}

// the host blob of fs_snapshot / fs_restore: this header, then the device blob
struct SnapHostHeader {
  uint64_t magic;            // SNAP_MAGIC
  uint64_t layout;           // fs_snapshot_info.layout of the handle it came from
  uint64_t dev_bytes;        // fs_snapshot_info.bytes
  int32_t after_reset;       // SimBase::after_reset
  int32_t reserved[9];
};
static_assert(sizeof(SnapHostHeader) == 64, "the device part of a host blob starts 16-byte aligned");
constexpr uint64_t SNAP_MAGIC = 0x31504E5357534C46ull;      // "FLSWSNP1"

inline uint64_t snap_hash(uint64_t h, uint64_t v) {         // FNV-1a over the 8 bytes of v
  for (int k = 0; k < 8; ++k) {
    h ^= (v >> (8 * k)) & 0xFFull;
    h *= 0x100000001B3ull;
  }
  return h;
}

}  // namespace fs
