// Device-side WAL recovery verify (tkv_wal_device.hip), used by tkv_wal_verify and
// tkv_wal_verify_device (tkv_wal_host.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tkv {

// Verify the WAL image [d_wal, d_wal + size) in device memory on `st` (synchronous): one sweep that
// walks the record chain and folds every payload of at most 64 KiB, device fix-up rounds where a
// chunk's speculative entry was wrong, one CRC batch for longer payloads, the first bad record. Same
// results as tkv_wal_verify. *needs_host_walk is set (and nothing else is decided) when the fix-up
// rounds have not settled the chain within their budget (kRoundBudget); the caller then runs the
// exact host walk.
int wal_verify_device_impl(const std::uint8_t* d_wal, std::uint64_t size, std::uint64_t* n_good,
                           std::uint64_t* stop_offset, hipStream_t st, bool* needs_host_walk);

// Host image: copied into a device buffer kept per device (pinned sources in one copy, pageable ones
// through pinned staging slabs filled by host threads), then wal_verify_device_impl. Sets
// *needs_host_walk also when the device cannot hold the image.
int wal_verify_host_image_impl(const std::uint8_t* h_wal, std::uint64_t size, std::uint64_t* n_good,
                               std::uint64_t* stop_offset, bool* needs_host_walk);

// wal_verify_device_impl, then the record index of the settled chain (tkv_wal_index_device): a scan of
// the per-region good-record counts and one more read of the image that writes the start offsets of
// the first min(*n_good, cap) good records, in chain order, to d_off64 / d_off32 (device; either may be
// null) and reduces the largest sequence_ among the good records. Status, *n_good and *stop_offset are
// the verify's. When *needs_host_walk is set nothing is indexed: the caller takes the positions from
// the exact host walk.
int wal_index_device_impl(const std::uint8_t* d_wal, std::uint64_t size, std::uint64_t* d_off64, std::uint32_t* d_off32,
                          std::uint64_t cap, std::uint64_t* n_good, std::uint64_t* stop_offset, std::uint64_t* max_sequence,
                          hipStream_t st, bool* needs_host_walk);

// Host image: copied as wal_verify_host_image_impl does, indexed on the device copy, the offsets copied
// back to h_off64 (host, cap entries).
int wal_index_host_image_impl(const std::uint8_t* h_wal, std::uint64_t size, std::uint64_t* h_off64, std::uint64_t cap,
                              std::uint64_t* n_good, std::uint64_t* stop_offset, std::uint64_t* max_sequence,
                              bool* needs_host_walk);

// The host image [h_wal, h_wal + size) into the caller's device buffer d_dst, as the host-image verify
// and index copy theirs (pinned sources in one copy, pageable ones through the pinned staging slabs);
// synchronous.
int wal_host_image_stage_impl(const std::uint8_t* h_wal, std::uint64_t size, std::uint8_t* d_dst);

// WAL resynchronisation on `st` (tkv_wal_resync.hip; synchronous): *found = the smallest p >= from
// (from <= size, checked by the caller) at which a record passes every check of wal_entry::decode,
// TKV_OK; or *found = size, TKV_NOT_FOUND. Counts into wal_salvage_last().
int wal_resync_device_impl(const std::uint8_t* d_wal, std::uint64_t size, std::uint64_t from, std::uint64_t* found,
                           hipStream_t st);

// d_off64[0, n) += base on `st` (asynchronous): a sub-image's index offsets made absolute.
int wal_salvage_add_base(std::uint64_t* d_off64, std::uint64_t n, std::uint64_t base, hipStream_t st);

// The calling thread's six salvage counters (tkv_debug_wal_salvage_last): resynchronisations, search
// spans, start offsets tested, candidates folded, their payload bytes, index calls.
std::uint64_t* wal_salvage_last();

}  // namespace tkv
