// Engine entry points shared by the C ABI files (tkv_crc32_host.cpp and the host format files
// tkv_wal_host.cpp, tkv_sst_host.cpp, tkv_runs_host.cpp), and the call structs of the format paths.
// Each engine entry point takes the checksum family (Algo) and works on the calling thread's current
// device; arguments and return codes are those of the matching tkv_crc32_* functions in
// include/tkv_crc32.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tkv_crc32.h"
#include "tkv_crc32_internal.h"

namespace tkv {

int update_impl(int algo, std::uint32_t raw_state, const void* data, std::size_t len, std::uint32_t* out_raw);
int update_device_impl(int algo, std::uint32_t raw_state, const void* d_data, std::size_t len,
                       std::uint32_t* d_out_raw, void* stream);
int batch_device_impl(int algo, const std::uint8_t* d_base, const std::uint64_t* d_offsets,
                      const std::uint32_t* d_lengths, const std::uint32_t* d_init_raw, std::uint32_t* d_out_final,
                      std::uint64_t n, void* stream);
int batch_uniform_impl(int algo, const std::uint8_t* d_base, std::uint64_t stride, std::uint64_t len,
                       const std::uint32_t* d_init_raw, std::uint32_t* d_out_final, std::uint64_t n, void* stream);
int batch_host_impl(int algo, const std::uint8_t* h_base, const std::uint64_t* h_offsets,
                    const std::uint32_t* h_lengths, const std::uint32_t* h_init_raw, std::uint32_t* h_out_final,
                    std::uint64_t n);
int batch_host_multi_impl(int algo, const int* devices, int ndev, const std::uint8_t* h_base,
                          const std::uint64_t* h_offsets, const std::uint32_t* h_lengths,
                          const std::uint32_t* h_init_raw, std::uint32_t* h_out_final, std::uint64_t n);

// Record `msg` as this thread's tkv_last_error() text; returns `code`.
int set_error(int code, const char* msg);
// Constant tables of `algo` on the current device (creates the device context); nullptr on error.
const DeviceTables* device_tables(int algo);
// Compute units of the current device (from its device context, created if need be); 0 on error.
int device_cu_count();

// tkv_crc32_kernels.hip: SSTable stamp fix-up (see tkv_sst_block_crcs_device).
hipError_t launch_sst_fix(std::uint8_t* file, const std::uint64_t* offsets, const std::uint32_t* sizes,
                          std::uint32_t* out, std::uint64_t n, int store, const DeviceTables* tabs, hipStream_t st);

// One call struct per format path: the arguments of its tkv_*[_device] pair in ABI order, built once by
// the extern "C" function and handed from the shared check to the host path or to the *_device_impl.

// The arguments of tkv_sst_build[_device] (include/tkv_crc32.h "SSTable flush").
struct SstBuildCall {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;
  std::uint64_t n;
  std::uint32_t target_block_size;
  std::uint8_t* file;
  std::uint64_t cap;
  std::uint64_t* block_off;
  std::uint32_t* block_size;
  std::uint32_t* block_first;
  std::uint64_t block_cap;
  std::uint64_t *file_size, *n_blocks, *index_offset, *index_size;
};

// tkv_sst_build.hip: the SSTable flush on `st` (synchronous): size scans, the exact block cut by pointer
// doubling, the host's invalid / overflow decision from a pinned result, the tile emit of blocks, index
// and footer with zero CRC fields, one CRC batch and the stamp. Arguments and results are
// tkv_sst_build_device's (n >= 1, target_block_size >= 1 and the required pointers checked by the caller).
int sst_build_device_impl(const SstBuildCall& c, hipStream_t st);

// The arguments of tkv_sst_scan[_device] (include/tkv_crc32.h "SSTable scan").
struct SstScanCall {
  const std::uint8_t* file;
  std::uint64_t file_size;
  std::uint32_t flags;
  std::uint64_t* key_off;
  std::uint32_t* key_len;
  std::uint64_t* val_off;
  std::uint32_t* val_len;
  std::uint64_t entry_cap;
  std::uint8_t* keys;
  std::uint64_t keys_cap;
  std::uint8_t* vals;
  std::uint64_t vals_cap;
  std::uint64_t* block_off;
  std::uint32_t* block_size;
  std::uint32_t* block_first;
  std::uint64_t block_cap;
  std::uint64_t *n_entries, *n_blocks, *keys_size, *vals_size, *bad_block;
};

// A scan's TKV_CORRUPTED: *bad_block = bad, the other results zero, `msg` the error text.
inline int sst_scan_corrupted(const SstScanCall& c, std::uint64_t bad, const char* msg) {
  *c.bad_block = bad;
  *c.n_entries = *c.n_blocks = *c.keys_size = *c.vals_size = 0;
  return set_error(TKV_CORRUPTED, msg);
}

// tkv_sst_scan.hip: the SSTable scan on `st` (synchronous): the footer's fields, the index chain by
// pointer doubling, one CRC batch over the block images and the footer's span, the wave-per-block parse
// through LDS windows, the host's corrupted / overflow decision from a pinned result, the records and the
// arena emit. Arguments and results are tkv_sst_scan_device's (pointers, flags and 28 <= file_size <=
// 2^32 - 1 checked by the caller).
int sst_scan_device_impl(const SstScanCall& c, hipStream_t st);

// The arguments of tkv_wal_encode[_device] (include/tkv_crc32.h "WAL group-commit encode").
struct WalEncodeCall {
  const std::uint8_t* keys;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint8_t* vals;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;
  const std::uint8_t* op;
  const std::uint8_t* tomb;
  const std::uint64_t* seq;
  std::uint64_t first_seq, n;
  std::uint8_t* img;
  std::uint64_t cap;
  std::uint64_t* rec_off;
  std::uint32_t* crc;
  std::uint64_t* img_size;
};

// tkv_wal_encode.hip: the WAL group-commit encode on `st` (synchronous): the size scan, the host's
// overflow / invalid decision from its pinned result, then the emit into [img, img + total) with the
// CRC of every record of record_len <= 240 folded in the same pass and the longer ones stamped by one
// CRC batch over the written image. Arguments and results are tkv_wal_encode_device's (n >= 1 and the
// required pointers checked by the caller).
int wal_encode_device_impl(const WalEncodeCall& c, hipStream_t st);

// The arguments of tkv_wal_decode_device (include/tkv_crc32.h "WAL batched decode"); tkv_wal_decode_host
// has no rec_off32.
struct WalDecodeCall {
  const std::uint8_t* img;
  std::uint64_t size;
  const std::uint64_t* rec_off64;
  const std::uint32_t* rec_off32;
  std::uint64_t n;
  std::uint32_t flags;
  std::uint8_t* op;
  std::uint8_t* tomb;
  std::uint64_t* seq;
  std::uint64_t* key_off;
  std::uint32_t* key_len;
  std::uint64_t* val_off;
  std::uint32_t* val_len;
  std::uint8_t* keys;
  std::uint64_t keys_cap;
  std::uint8_t* vals;
  std::uint64_t vals_cap;
  std::uint64_t *keys_size, *vals_size, *first_bad;
};

// tkv_wal_decode.hip: the batched WAL decode on `st` (synchronous): the header pass as level 0 of the key
// and value length scans, the host's corrupted / overflow decision from its pinned result, then the
// columns, the arena offsets and the emit of every copied arena. Arguments and results are
// tkv_wal_decode_device's (n >= 1, the flags, the offset arrays and the required pointers checked by
// the caller, who also presets *keys_size = *vals_size = 0).
int wal_decode_device_impl(const WalDecodeCall& c, hipStream_t st);

// The arguments of tkv_memtable_build[_device] (include/tkv_crc32.h "Memtable replay").
struct MemtableCall {
  const std::uint8_t* keys;
  std::uint64_t keys_size;
  const std::uint64_t* key_off;
  const std::uint32_t* key_len;
  const std::uint64_t* val_off;
  const std::uint32_t* val_len;
  const std::uint8_t* op;
  const std::uint8_t* tomb;
  const std::uint64_t* seq;
  std::uint64_t n, timestamp_ms;
  std::uint8_t* ikeys;
  std::uint64_t ikeys_cap;
  std::uint64_t* ikey_off;
  std::uint32_t* ikey_len;
  std::uint64_t* out_val_off;
  std::uint32_t* out_val_len;
  std::uint32_t* src;
  std::uint64_t entry_cap;
  std::uint64_t *n_entries, *ikeys_size, *first_bad;
};

// tkv_memtable.hip: the memtable replay on `st` (synchronous): the checks and first comparison words,
// rounds of a stable LSD radix sort over the unresolved records, the dedupe scans, the host's corrupted /
// invalid / overflow decision from a pinned result, the columns and the tile emit of the internal keys.
// Arguments and results are tkv_memtable_build_device's (1 <= n <= 2^32 - 1 and the required pointers
// checked by the caller).
int memtable_build_device_impl(const MemtableCall& c, hipStream_t st);

// The arguments of tkv_sst_merge[_device] (include/tkv_crc32.h "SSTable merge"): the per-run arrays are
// host arrays of n_runs elements in both calls.
struct SstMergeCall {
  std::uint32_t n_runs;
  const std::uint8_t* const* keys;
  const std::uint64_t* keys_size;
  const std::uint64_t* const* key_off;
  const std::uint32_t* const* key_len;
  const std::uint64_t* const* val_off;  // nullable, and every element nullable
  const std::uint32_t* const* val_len;
  const std::uint64_t* n;
  const std::uint8_t* key_base;
  const std::uint64_t* val_bias;  // nullable: zeros
  std::uint32_t flags;
  std::uint64_t* out_key_off;
  std::uint32_t* out_key_len;
  std::uint64_t* out_val_off;
  std::uint32_t* out_val_len;
  std::uint64_t* out_src;
  std::uint64_t entry_cap;
  std::uint64_t *n_entries, *keys_bytes, *vals_bytes, *first_bad;
};

// tkv_sst_merge.hip: the k-way merge on `st` (synchronous): the check pass with the sort entries, the
// merge-path rounds, the ties and the survivor scan, the host's corrupted / overflow decision from a pinned
// result, the columns. Arguments and results are tkv_sst_merge_device's (the argument checks made and
// 1 <= N <= 2^32 - 1 by the caller).
int sst_merge_device_impl(const SstMergeCall& c, hipStream_t st);

// The arguments of tkv_sst_get[_device] (include/tkv_crc32.h "SSTable get"): the per-run arrays are host
// arrays of n_runs elements in both calls, as the merge's.
struct SstGetCall {
  std::uint32_t n_runs;
  const std::uint8_t* const* keys;
  const std::uint64_t* keys_size;
  const std::uint64_t* const* key_off;
  const std::uint32_t* const* key_len;
  const std::uint64_t* const* val_off;  // nullable, and every element nullable
  const std::uint32_t* const* val_len;
  const std::uint64_t* n;
  const std::uint8_t* const* vals;  // nullable: no gather, no value span check
  const std::uint64_t* vals_size;
  const std::uint64_t* val_bias;    // nullable: zeros
  const std::uint8_t* qkeys;
  std::uint64_t qkeys_size;
  const std::uint64_t* q_off;
  const std::uint32_t* q_len;
  std::uint64_t nq;
  std::uint32_t flags;
  std::uint8_t* state;
  std::uint64_t* src;
  std::uint64_t* seq;
  std::uint64_t* out_val_off;
  std::uint32_t* out_val_len;
  std::uint64_t* out_val_pos;
  std::uint8_t* out_vals;
  std::uint64_t vals_cap;
  std::uint64_t *n_found, *vals_bytes, *first_bad;
};

// tkv_sst_get.hip: the batched point lookup on `st` (synchronous): the query check and the per-run
// upper-bound searches of one lane per query, the scans of the found flags and the value lengths, the
// host's invalid / corrupted / overflow decision from a pinned result, the columns and the value gather.
// Arguments and results are tkv_sst_get_device's (the argument checks made and 1 <= nq <= 2^32 - 1 by the
// caller).
int sst_get_device_impl(const SstGetCall& c, hipStream_t st);

}  // namespace tkv
