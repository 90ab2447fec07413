/*
 * tkv_crc32.h — C ABI of the MI355X CRC-32 block-checksum engine (libtkv_crc32.so).
 *
 * Drop-in boundary for tinykvpp's integrity hot path: the CRC-32/ISO-HDLC routine
 * frankie::core::crc32 (/root/reference/src/core/crc32.hpp:32-49, crc32.cpp:9-22) and the call
 * sites that stamp/verify WAL records (/root/reference/src/engine/wal.cpp:54-58, 89-96).
 * Plain C: pointers, sizes and integer status codes only. Every batch, device and host-pipeline
 * entry point computes on the HIP kernels for gfx950 and reports TKV_IO_ERROR when no GPU is usable;
 * none of them falls back to the CPU. The CPU computes only in the separately named single-span
 * entry points tkv_crc32[c]_update_host and tkv_crc32[c]_update_fallback, which the drop-in header
 * include/frankie_crc32.hpp uses to keep crc32::update's never-fail contract (crc32.cpp:9-16).
 *
 * State conventions (match crc32.hpp:37-46):
 *   "raw" register  = the value crc32::crc_ holds (init 0xFFFFFFFF, no xorout applied);
 *   "final" value   = crc32::finalize() = raw ^ 0xFFFFFFFF.
 *
 * Stream arguments are hipStream_t passed as void* (NULL = the legacy default stream).
 */
#ifndef TKV_CRC32_H
#define TKV_CRC32_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes mirror frankie::core::status_code (/root/reference/src/core/status.hpp:11-20). */
enum tkv_status {
  TKV_OK = 0,
  TKV_NOT_FOUND = 1,
  TKV_IO_ERROR = 2,          /* HIP runtime failure (no device, launch or copy error) */
  TKV_INVALID_ARGUMENT = 3,
  TKV_CORRUPTED = 4,         /* a verified checksum did not match (wal.cpp:93-96) */
  TKV_EOF = 5,
  TKV_OUT_OF_MEMORY = 6,
  TKV_BUFFER_OVERFLOW = 7
};

#define TKV_CRC32_DEFAULT_RAW 0xFFFFFFFFu /* crc32.hpp:9 kCRC32DefaultValue */
#define TKV_CRC32_POLYNOMIAL 0xEDB88320u  /* crc32.hpp:11 kCRC32Polynomial */

/* ---- library / device management -------------------------------------------------------------- */

/* Number of usable GPUs (0 when the HIP runtime finds none). */
int tkv_device_count(void);

/* Bind the calling thread to `device` and create that device's context (tables, scratch) if needed.
 * Every other entry point uses the calling thread's current device. */
int tkv_set_device(int device);

/* Human-readable text of the last error on this thread ("" if none). */
const char *tkv_last_error(void);

/* Build identity: 16 hex digits of sha256 over the library's sources and Makefile, baked in at build
 * time (tinykvpp_amd/build_id.py); tests and bench.py check it against the tree they run in. */
const char *tkv_build_id(void);

/* ---- crc32::update replacement ---------------------------------------------------------------- */

/* Continue raw register `raw_state` over `len` bytes of HOST memory; writes the new raw register.
 * Replaces crc32::update (crc32.hpp:37, crc32.cpp:9-16); finalize is raw ^ 0xFFFFFFFF
 * (crc32.cpp:19) and reset is raw = 0xFFFFFFFF (crc32.cpp:22). Synchronous (stages through the
 * GPU; the right tool for one span is the batch API). */
int tkv_crc32_update(uint32_t raw_state, const void *data, size_t len, uint32_t *out_raw);

/* Same over DEVICE memory, asynchronous on `stream`; *d_out_raw is written on the device. */
int tkv_crc32_update_device(uint32_t raw_state, const void *d_data, size_t len, uint32_t *d_out_raw,
                            void *stream);

/* Host-CPU latency path for ONE short span (slicing-by-8; no device, never fails on valid
 * arguments): the same register semantics as tkv_crc32_update. No other entry point calls it. The
 * drop-in header include/frankie_crc32.hpp routes spans of at most TKV_DROPIN_HOST_MAX bytes here
 * (default 65536, the measured host/GPU crossover of one call), which covers the reference's per-put
 * record stamp (wal.cpp:54-57): 0.011 us for 36 bytes against ~11 us for a GPU round trip
 * (INTEGRATION.md §1). */
int tkv_crc32_update_host(uint32_t raw_state, const void *data, size_t len, uint32_t *out_raw);
int tkv_crc32c_update_host(uint32_t raw_state, const void *data, size_t len, uint32_t *out_raw);

/* The drop-in header's recovery after tkv_crc32[c]_update returned `gpu_status` != TKV_OK: the same
 * span recomputed on the host (the slicing-by-8 code of tkv_crc32_update_host), so crc32::update
 * keeps the reference's never-fail contract (crc32.cpp:9-16) for spans of any size on a node without
 * a usable GPU. Prints one warning per process on stderr (with gpu_status and tkv_last_error()) and
 * counts the call in tkv_debug_update_counts_n out[2]. Fails only on null pointers. */
int tkv_crc32_update_fallback(int gpu_status, uint32_t raw_state, const void *data, size_t len, uint32_t *out_raw);
int tkv_crc32c_update_fallback(int gpu_status, uint32_t raw_state, const void *data, size_t len,
                               uint32_t *out_raw);

/* CRC of the concatenation A || B from crc1 = CRC(A), crc2 = CRC(B) (finalized values) and
 * len2 = |B| (zlib's crc32_combine): Shift_len2(crc1) ^ crc2, GF(2) arithmetic on the 4-byte
 * values only (host, no data, no device). The reference has no equivalent; it serves callers that
 * checksum the pieces of one record or file separately (the multi-device batch does this itself). */
uint32_t tkv_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* ---- batch APIs (new: the reference has only per-record calls, wal.cpp:54-57,89-92) ------------ */

/* Irregular batch in device memory: block i is [d_base + d_offsets[i], + d_lengths[i]) (any
 * alignment, any length, blocks may overlap). d_out_final[i] = finalize() of the block continued
 * from d_init_raw[i] (NULL: every block starts from 0xFFFFFFFF). Asynchronous on `stream`; d_* must
 * stay valid until the stream has completed. */
int tkv_crc32_batch_device(const uint8_t *d_base, const uint64_t *d_offsets, const uint32_t *d_lengths,
                           const uint32_t *d_init_raw, uint32_t *d_out_final, uint64_t n, void *stream);

/* Uniform batch in device memory: block i is [d_base + i*stride, + len). Fast path for fixed-size
 * WAL/SSTable blocks (no prepass; 16-byte aligned blocks take the aligned kernel). */
int tkv_crc32_batch_uniform_device(const uint8_t *d_base, uint64_t stride, uint64_t len,
                                   const uint32_t *d_init_raw, uint32_t *d_out_final, uint64_t n,
                                   void *stream);

/* Irregular batch in HOST memory on the current device: blocks are streamed through pinned
 * staging buffers with H2D copy / kernel / D2H copy overlapped on two streams. Synchronous.
 * h_base may be pageable or pinned: when every block lies inside one pinned allocation mapped at
 * the same address on the device (hipHostMalloc, hipHostRegister), the kernels read the blocks in
 * place over PCIe and only offsets, lengths and results are copied. */
int tkv_crc32_batch_host(const uint8_t *h_base, const uint64_t *h_offsets, const uint32_t *h_lengths,
                         const uint32_t *h_init_raw, uint32_t *h_out_final, uint64_t n);

/* Same, split across `ndev` devices by bytes (one host thread and stream pair per device, no
 * collective). A block of at least 1 MiB that straddles the boundary between two devices' byte
 * shares is cut there; its pieces run on both devices and their registers combine on the host
 * (tkv_crc32_combine), so one huge block also spreads over the devices. */
int tkv_crc32_batch_host_multi(const int *devices, int ndev, const uint8_t *h_base, const uint64_t *h_offsets,
                               const uint32_t *h_lengths, const uint32_t *h_init_raw, uint32_t *h_out_final,
                               uint64_t n);

/* ---- WAL record verification (wal_entry::decode's CRC check, wal.cpp:63-96) ------------------- */

/* Verify every record of a slurped WAL image (host memory, wal_reader::open, wal.cpp:204-240):
 * copies it to the device, walks the record_len chain and checks all CRCs there, and reports the
 * number of leading good records in *n_good and the byte offset where decoding stopped in
 * *stop_offset. Returns TKV_OK when the whole image verified (clean EOF), TKV_CORRUPTED at the
 * first record whose length or CRC is bad (wal.cpp:68-96 order: header size, length, CRC). */
int tkv_wal_verify(const uint8_t *h_wal, uint64_t size, uint64_t *n_good, uint64_t *stop_offset);

/* Same for a WAL image already in DEVICE memory (synchronous on `stream`). The record_len chain is
 * walked on the device (speculative parallel walk, exact stitching), then one CRC batch and a
 * first-corruption search; results and status as tkv_wal_verify. tkv_wal_verify itself copies the
 * host image to the device and takes this path (host-thread walk only as the exact fallback). */
int tkv_wal_verify_device(const uint8_t *d_wal, uint64_t size, uint64_t *n_good, uint64_t *stop_offset,
                          void *stream);

/* Check n records of a WAL image already in DEVICE memory whose start offsets are known - the record
 * list of a walk, or the offsets a group-commit writer kept: record i starts at
 * d_img + d_rec_off[i] (u32 offsets, images up to 4 GiB). Each record gets wal_entry::decode's checks
 * (wal.cpp:63-127): at least 26 bytes left, record_len + 8 within the image, the CRC-32 of the
 * record_len payload bytes equal to the stored CRC, key and value inside the payload. The payload
 * length comes from the record's own header, read from the same 16-byte granules as its payload: no
 * lengths array, no prepass. *d_first_bad (device memory) = the index of the first record failing a
 * check, n when every record passes. d_crc (nullable, device): the computed finalized CRC of every
 * payload (0 for a record whose length check failed). max_payload is a dispatch hint (the longest
 * record_len the caller expects: one lane reads each record in a window of 4-8 16-byte granules sized
 * for it, 36-byte payloads in 4, up to 100 bytes in 8); longer payloads are still checked exactly,
 * 64 bytes at a time. Asynchronous on `stream`. */
int tkv_wal_check_records_device(const uint8_t *d_img, uint64_t size, const uint32_t *d_rec_off, uint64_t n,
                                 uint32_t max_payload, uint32_t *d_crc, uint64_t *d_first_bad, void *stream);

/* Verify the image as tkv_wal_verify_device does and also list its good records: what the recovery
 * loop of engine::create needs besides the verdict (engine.cpp:31-53: every good record goes to the
 * memtable, and the next sequence number is the largest one seen plus 1).
 * d_off64 / d_off32 (device, either or both may be NULL): start offset of good record i, in chain
 * order, for i < min(*n_good, cap). Entries at and after that index are not written. cap > 0 with both
 * NULL, and d_off32 with size > 4 GiB, are TKV_INVALID_ARGUMENT. *n_good is the full count also when
 * cap is smaller; cap == 0 is a verify that additionally returns *max_sequence.
 * *max_sequence: the largest sequence_ field (u64 LE at record byte 9) over the good records,
 * 0 when there are none (engine.cpp:17,46).
 * Status, *n_good, *stop_offset: identical to tkv_wal_verify_device on the same image. The chain the
 * verify settled is scanned (per-region record counts) and the image read once more to write the
 * offsets out; d_off32 is the list tkv_wal_check_records_device takes. Synchronous on `stream`. */
int tkv_wal_index_device(const uint8_t *d_wal, uint64_t size, uint64_t *d_off64, uint32_t *d_off32, uint64_t cap,
                         uint64_t *n_good, uint64_t *stop_offset, uint64_t *max_sequence, void *stream);

/* Host image (pageable or pinned): copied to the device as tkv_wal_verify does, indexed there, the
 * offsets of the first min(*n_good, cap) good records copied back to h_off64 (cap entries; may be NULL
 * when cap is 0). */
int tkv_wal_index(const uint8_t *h_wal, uint64_t size, uint64_t *h_off64, uint64_t cap, uint64_t *n_good,
                  uint64_t *stop_offset, uint64_t *max_sequence);

/* ---- WAL salvage: resynchronise past corrupted records ------------------------- */

/* Everything above stops at the first bad record, as wal_entry::decode and engine::create do. The calls
 * below go on behind it. valid(p), for an image [0, size), holds when (all arithmetic 64-bit)
 *   1. size - p >= 26;
 *   2. rl + 8 <= size - p, rl the u32 LE at p;
 *   3. 18 + kl + vl <= rl, kl and vl the u32 LE at p + 18 and p + 22;
 *   4. the finalized CRC-32 of bytes [p + 8, p + 8 + rl) equals the u32 LE at p + 4
 * - the checks of tkv_wal_check_records_device. The salvage of an image is the sequential program
 *     p = 0; while p < size: if valid(p): emit record p, p += 8 + rl(p); else: p is skipped, p += 1
 * and a gap [a, b) is a maximal run of skipped bytes (b == size: a tail gap). Two consequences of the
 * definition: a candidate that passes by CRC collision (2^-32 per structurally plausible candidate) is
 * accepted, and so are valid records nested inside a corrupted record's value (their bytes are in a
 * skipped range). Cost: every byte offset of a damaged range is tested (checks 1-3), and each survivor
 * costs the CRC of its record_len bytes; a crafted image whose damaged range is dense with plausible
 * headers and long record_len values costs candidates x payload bytes of CRC work, which a sequential
 * salvage pays as well. */

/* Smallest p >= from with valid(p). TKV_OK and *found = p; TKV_NOT_FOUND and *found = size when there
 * is none (from == size included). from > size, NULL d_wal with size > 0, NULL found:
 * TKV_INVALID_ARGUMENT, decided before any device work. Synchronous on `stream`. No byte outside the
 * 16-byte granules of [d_wal, d_wal + size) is read, whatever the header fields say. No CRC on the CPU;
 * no usable GPU: TKV_IO_ERROR. The search runs in spans of start offsets from `from` (64 KiB first,
 * four times longer each, 16 MiB at most); structurally plausible candidates are checked in offset
 * order in batches of bounded payload bytes, and the search ends with the batch that holds the answer. */
int tkv_wal_resync_device(const uint8_t *d_wal, uint64_t size, uint64_t from, uint64_t *found, void *stream);

/* The salvage program above, as a loop of tkv_wal_index_device on the sub-image [p, size) and
 * tkv_wal_resync_device from its stop offset + 1.
 * d_off64 (device, cap entries, nullable when cap == 0): start offsets, absolute in the image, of the
 *   first min(*n_records, cap) salvaged records in increasing order; *n_records is the full count.
 * h_gaps (host, 2 * gap_cap u64, nullable when gap_cap == 0): {start, end} of the first
 *   min(*n_gaps, gap_cap) gaps; *n_gaps is the full count.
 * max_gaps: at most this many resynchronisations. On meeting invalid position g with max_gaps gaps
 *   already closed the call stops: *stop_offset = g, and the records and gaps listed are those before g.
 *   Otherwise *stop_offset = size. With max_gaps == 0 status, *n_records, *stop_offset, *max_sequence
 *   and the offsets are exactly tkv_wal_index_device's on the same image.
 * *max_sequence: largest sequence_ over the salvaged records, 0 for none.
 * *bytes_skipped: sum of the closed gaps' lengths, listed or not.
 * TKV_OK iff *n_gaps == 0 and *stop_offset == size (then identical to a clean index); else
 * TKV_CORRUPTED with every output valid. Argument errors as tkv_wal_index_device (and gap_cap > 0 with
 * NULL h_gaps), decided first. When the index of a sub-image hands over to the exact host walk (its
 * fix-up round budget), that walk's records are taken and the salvage stops resynchronising there:
 * *stop_offset is that stop, the status TKV_CORRUPTED. Synchronous on `stream`. */
int tkv_wal_salvage_device(const uint8_t *d_wal, uint64_t size, uint64_t *d_off64, uint64_t cap,
                           uint64_t *h_gaps, uint64_t gap_cap, uint64_t max_gaps, uint64_t *n_records,
                           uint64_t *n_gaps, uint64_t *stop_offset, uint64_t *bytes_skipped,
                           uint64_t *max_sequence, void *stream);

/* Host image (pageable or pinned): copied to the device the way tkv_wal_index copies it, salvaged
 * there, the offsets copied back to h_off64 (cap entries; may be NULL when cap is 0). The device copies
 * of the image and of the offsets are kept per device between calls, up to 256 MiB each, and the work
 * runs on a stream of the library's own; calls on one device take turns. When the device
 * cannot hold the image or its offsets, the result is tkv_wal_index's (its exact host walk) with
 * *stop_offset at its stop, *n_gaps = 0, and nothing is resynchronised; likewise behind a sub-image
 * whose index used up its round budget (above). */
int tkv_wal_salvage(const uint8_t *h_wal, uint64_t size, uint64_t *h_off64, uint64_t cap, uint64_t *h_gaps,
                    uint64_t gap_cap, uint64_t max_gaps, uint64_t *n_records, uint64_t *n_gaps,
                    uint64_t *stop_offset, uint64_t *bytes_skipped, uint64_t *max_sequence);

/* Stamp n records in place (host memory): for record i at h_buf + h_offsets[i] of total size
 * h_sizes[i] (>= 8), write crc32 of bytes [8, size) LE at offset 4 (wal.cpp:54-58). */
int tkv_wal_stamp(uint8_t *h_buf, const uint64_t *h_offsets, const uint32_t *h_sizes, uint64_t n);

/* ---- WAL group-commit encode (batch encode) ------------------------------- */

/* wal_entry::encode (wal.cpp:19-61) for a batch of n records held as arenas: key i is
 * [keys + key_off[i], + key_len[i]), value i is [vals + val_off[i], + val_len[i]). Sources may have any
 * alignment, may have gaps and may overlap each other (many records may share one key); they do not
 * overlap the destination. Record i is written exactly as the reference writes it, little-endian:
 *     u32 record_len = 18 + key_len + val_len | u32 crc32 | u8 op | u64 seq | u8 tombstone |
 *     u32 key_len | u32 val_len | key | value
 * with crc32 the finalized CRC-32 of bytes [8, 26 + key_len + val_len) (wal.cpp:54-58). Records lie
 * back to back in batch order, record 0 at img[0].
 * Defaults: val_len == NULL: every value is empty (vals / val_off ignored); op == NULL: every op byte
 * 0 (put); tomb == NULL: every tombstone byte 0; seq == NULL: seq[i] = first_seq + i (otherwise
 * first_seq is ignored). The tombstone byte is written as 0 or 1 (nonzero input becomes 1), the op
 * byte as given.
 * img may have any byte alignment (a caller appends at the tail of an image it holds); no byte outside
 * [img, img + total) is written or read-modify-written, total = sum of (26 + key_len + val_len).
 * *img_size = total whenever the arguments are valid. total > cap: TKV_BUFFER_OVERFLOW, and nothing is
 * written to img, rec_off or crc (cap = 0 with img = NULL is the sizing call). 18 + key_len + val_len
 * beyond u32 for some record: TKV_INVALID_ARGUMENT, nothing written, no source byte read (the
 * reference would wrap silently). rec_off (nullable): start offset of record i, n entries. crc
 * (nullable): the stamped CRC of record i. n == 0: TKV_OK, *img_size = 0, nothing touched.
 * n > 2^32 - 1, or NULL where a pointer is required (keys, key_off, key_len, img_size; vals and
 * val_off with val_len): TKV_INVALID_ARGUMENT.
 * The device call is synchronous on `stream` (the host needs total before the emit); with no usable
 * GPU it returns TKV_IO_ERROR. No CRC is computed on the CPU in either call. */
int tkv_wal_encode_device(const uint8_t *d_keys, const uint64_t *d_key_off, const uint32_t *d_key_len,
                          const uint8_t *d_vals, const uint64_t *d_val_off, const uint32_t *d_val_len,
                          const uint8_t *d_op, const uint8_t *d_tomb, const uint64_t *d_seq, uint64_t first_seq,
                          uint64_t n, uint8_t *d_img, uint64_t cap, uint64_t *d_rec_off, uint32_t *d_crc,
                          uint64_t *img_size, void *stream);

/* The same with every argument in HOST memory. Sizes and offsets are computed and the records laid
 * out (CRC fields zero) on host threads; the CRCs come from the path tkv_wal_stamp uses (pinned
 * memory is read in place), then the fields are stored. Sizing, overflow and argument errors are
 * decided before any GPU call. */
int tkv_wal_encode(const uint8_t *h_keys, const uint64_t *h_key_off, const uint32_t *h_key_len,
                   const uint8_t *h_vals, const uint64_t *h_val_off, const uint32_t *h_val_len,
                   const uint8_t *h_op, const uint8_t *h_tomb, const uint64_t *h_seq, uint64_t first_seq,
                   uint64_t n, uint8_t *h_img, uint64_t cap, uint64_t *h_rec_off, uint32_t *h_crc,
                   uint64_t *img_size);

/* ---- WAL batched decode (the inverse of the encode above) --------------------------------------- */

#define TKV_WAL_DECODE_KEY_VIEWS 1u   /* keys stay in the image */
#define TKV_WAL_DECODE_VAL_VIEWS 2u   /* values stay in the image */

/* The fields wal_entry::decode (wal.cpp:98-127) takes out of a record, for n records of an image in
 * DEVICE memory whose start offsets are known, in the columnar form tkv_wal_encode_device takes. Record
 * i starts at d_img + rec_off[i]; exactly one of d_rec_off64 (the list tkv_wal_index_device writes) and
 * d_rec_off32 (size <= 4 GiB) is non-NULL. The offsets need not be in chain order, may repeat, and the
 * records may overlap one another: this is a gather.
 * Columns (device, n entries, each nullable and then skipped): op[i] = byte 8 and tomb[i] = byte 17 as
 * stored, seq[i] = u64 LE at byte 9, key_len[i] / val_len[i] = u32 LE at bytes 18 / 22.
 * Key arena: record i's key is image bytes [rec_off[i] + 26, + key_len[i]). Without
 * TKV_WAL_DECODE_KEY_VIEWS the keys are written back to back in batch order into d_keys, key_off[i] is
 * the exclusive u64 prefix sum of key_len and *keys_size the sum. With it nothing is copied, d_keys /
 * keys_cap are ignored, key_off[i] = rec_off[i] + 26 and *keys_size is still the sum. Value arena: the
 * same with TKV_WAL_DECODE_VAL_VIEWS, d_vals and val_off[i]; the source is rec_off[i] + 26 +
 * key_len[i]. Bytes of a record behind its value (record_len > 18 + key_len + val_len) are ignored, as
 * the reference ignores them (wal.cpp:118-125).
 * In either mode the outputs are valid tkv_wal_encode_device inputs with keys / vals = the arena, or
 * = d_img for a views arena; when every record has the shape the reference encoder writes (record_len
 * == 18 + key_len + val_len, tombstone byte 0 or 1) encoding them reproduces the records byte for
 * byte, CRC field included.
 * Per record, wal_entry::decode's structural checks in 64-bit arithmetic: at least 26 bytes left at
 * rec_off[i] (wal.cpp:68), record_len + 8 within the image (:83), 18 + key_len + val_len <= record_len
 * (:118-121). NO CHECKSUM IS COMPUTED: that is the business of tkv_wal_index[_device] and
 * tkv_wal_check_records_device, which produce or check the offsets this call takes. No byte outside
 * [d_img, d_img + size) is read for any input, and the lengths of a record that fails a check are never
 * used as copy lengths. If any record fails: TKV_CORRUPTED, *first_bad = the smallest failing index,
 * *keys_size = *vals_size = 0 and nothing is written to any output array (a caller that wants the
 * prefix calls again with n = *first_bad). Otherwise *first_bad = n.
 * *keys_size > keys_cap for a copied arena, or the same for values: TKV_BUFFER_OVERFLOW; both sizes are
 * reported and nothing is written to any output array, columns included (caps of 0 with NULL arenas is
 * the sizing call). A copied arena whose total is 0 may be NULL. d_keys / d_vals may have any byte
 * alignment; no byte outside [d_keys, d_keys + *keys_size) and [d_vals, d_vals + *vals_size) is written
 * or read-modify-written; destinations do not overlap the image.
 * TKV_INVALID_ARGUMENT, decided before any device work: n > 2^32 - 1, both or neither offset array,
 * d_rec_off32 with size > 4 GiB, unknown flag bits, NULL d_img with n > 0, NULL keys_size / vals_size /
 * first_bad. n == 0: TKV_OK, sizes 0, *first_bad = 0, nothing else touched.
 * Synchronous on `stream` (the host needs the totals and first_bad before the emit); with no usable GPU
 * it returns TKV_IO_ERROR. */
int tkv_wal_decode_device(const uint8_t *d_img, uint64_t size, const uint64_t *d_rec_off64,
                          const uint32_t *d_rec_off32, uint64_t n, uint32_t flags, uint8_t *d_op, uint8_t *d_tomb,
                          uint64_t *d_seq, uint64_t *d_key_off, uint32_t *d_key_len, uint64_t *d_val_off,
                          uint32_t *d_val_len, uint8_t *d_keys, uint64_t keys_cap, uint8_t *d_vals,
                          uint64_t vals_cap, uint64_t *keys_size, uint64_t *vals_size, uint64_t *first_bad,
                          void *stream);

/* The same contract with every argument in HOST memory (u64 offsets only): the decode for an image the
 * caller holds on the host, paired with tkv_wal_index. It is NOT a fallback of the device call: the
 * field extraction and the arena copies run on host threads, no GPU is used and no checksum is
 * computed. */
int tkv_wal_decode_host(const uint8_t *h_img, uint64_t size, const uint64_t *h_rec_off64, uint64_t n, uint32_t flags,
                        uint8_t *h_op, uint8_t *h_tomb, uint64_t *h_seq, uint64_t *h_key_off, uint32_t *h_key_len,
                        uint64_t *h_val_off, uint32_t *h_val_len, uint8_t *h_keys, uint64_t keys_cap,
                        uint8_t *h_vals, uint64_t vals_cap, uint64_t *keys_size, uint64_t *vals_size,
                        uint64_t *first_bad);

/* ---- SSTable data-block stamping (the format is defined here) ----------- */

/* The reference writes sstable_data_block_header::crc32_ = 0 (sstable_writer.cpp:138-144) and never
 * reads it (sstable_reader.cpp:61-89), so this stamp is this library's format decision, not
 * reference behaviour ("parity unpinned"). A data-block image as get_data_block builds it
 * (sstable_writer.cpp:150-168) is varint(20) | header[20] | varint(n) | body[n], padded to the size
 * the index entry records (index_entry::data_block_size_, sstable_format.hpp:117-121); the header's
 * crc32_ field (sstable_format.hpp:97) therefore sits at image byte TKV_SST_CRC_OFFSET. The stamp is
 * the CRC-32 of the whole image [0, size) with those 4 bytes read as zero, stored little-endian in
 * the field. Images must be at least TKV_SST_MIN_IMAGE bytes and shorter than 4 GiB. */
#define TKV_SST_CRC_OFFSET 17u
#define TKV_SST_MIN_IMAGE 22u

/* Stamp n data-block images in place in a host buffer (an SSTable file image being written). */
int tkv_sst_stamp_blocks(uint8_t *h_file, const uint64_t *h_offsets, const uint64_t *h_sizes, uint64_t n);

/* Verify n images of a host buffer; *n_bad = number of mismatching images, *first_bad = index of
 * the first (n when none). Returns TKV_OK or TKV_CORRUPTED (read_data_block's corrupted status,
 * sstable_reader.cpp:73-86). */
int tkv_sst_verify_blocks(const uint8_t *h_file, const uint64_t *h_offsets, const uint64_t *h_sizes, uint64_t n,
                          uint64_t *n_bad, uint64_t *first_bad);

/* Device-resident images: d_out[i] = the stamp value of image i (CRC with the field read as zero),
 * whatever the field holds now. With store != 0 the value is also written into the field (stamping
 * on the device). Asynchronous on `stream`. */
int tkv_sst_block_crcs_device(uint8_t *d_file, const uint64_t *d_offsets, const uint32_t *d_sizes, uint32_t *d_out,
                              uint64_t n, int store, void *stream);

/* ---- SSTable index image + footer stamping (format defined here; parity unpinned) ------------------
 * research/12-integrity-crash-consistency.md §5 asks for a checksum over the index image and the
 * footer, kept in the footer's existing crc32_ field (sstable_format.hpp:129-135). The reference
 * writes only 8 footer bytes (kFooterSize, sstable_format.hpp:140), and in the order
 * (index_size, index_offset) (sstable_writer.cpp get_footer) while decode_footer reads
 * (index_offset, index_size) (sstable_format.cpp:99-106). The footer here is the full 20-byte struct
 * in declaration order, little-endian:
 *     u32 index_offset | u32 index_size | u32 bloom_offset | u32 bloom_size | u32 crc32_
 * and crc32_ = CRC-32 of (index image || footer bytes [0, 16)), i.e. the index bytes as get_index
 * lays them out (sstable_writer.cpp get_index) followed by the footer's first four fields. */
#define TKV_SST_FOOTER_SIZE 20u
#define TKV_SST_FOOTER_CRC_OFFSET 16u

/* Write the crc32_ field of h_footer (20 bytes; its first 16 bytes already filled) from the index
 * image [h_index, h_index + index_size) (index_size may be 0). */
int tkv_sst_stamp_footer(const uint8_t *h_index, uint64_t index_size, uint8_t *h_footer);

/* Check the stored crc32_ of h_footer against the index image: TKV_OK or TKV_CORRUPTED. */
int tkv_sst_verify_footer(const uint8_t *h_index, uint64_t index_size, const uint8_t *h_footer);

/* ---- SSTable flush: data blocks, index and footer in one call ------------------- */

/* The writer loop sstable_writer::append / is_data_block_complete / get_data_block / record_data_block /
 * get_index / get_footer (sstable_writer.cpp) for n entries held as arenas: internal key i is
 * [keys + key_off[i], + key_len[i]), value i is [vals + val_off[i], + val_len[i]). Entries are taken in
 * the order given; the call neither sorts them nor checks their order, as the reference writer does
 * not. Sources may have any alignment, may have gaps and may overlap each other (many entries may share
 * one key); they do not overlap the destination. val_len == NULL: every value is empty (vals / val_off
 * ignored).
 * Sizes. kl, vl = the lengths of entry i, vlen(x) = the bytes of LEB128(x). append counts
 * e_i = 8 + kl + vl per entry (sstable_writer.cpp:61,122) while write_string twice writes
 * w_i = vlen(kl) + kl + vlen(vl) + vl. S and W are the exclusive prefix sums of e and w.
 * Cut (append, then is_data_block_complete: size >= target, sstable_writer.cpp:127-129): b_0 = 0 and
 * b_{j+1} = the smallest m > b_j with S[m] - S[b_j] >= target_block_size, or n when there is none (the
 * trailing partial block). Block j holds the c_j entries [b_j, b_{j+1}) and counts z_j = S[b_{j+1}] -
 * S[b_j] bytes; B = the number of blocks.
 * Block image j, 36 + z_j bytes at file offset O_j = 36 * j + S[b_j], is the image the stamping section
 * above defines: 0x14 | u32 c_j | u32 z_j | u32 z_j | u8 0 | 3 zero bytes | u32 crc32_ | varint(z_j) |
 * the entries back to back as varint(kl) | key | varint(vl) | value (entry i at O_j + 21 + vlen(z_j) +
 * W[i] - W[b_j]) | zeros up to 36 + z_j (the slack between what is counted and what is written, and the
 * image padding). crc32_ is the stamp of tkv_sst_stamp_blocks.
 * Index image at index_offset = 36 * B + S[n]: u64 B, then per block varint(kl of entry b_j) | that key |
 * u64 O_j | u64 (36 + z_j) (get_index). Footer, 20 bytes directly behind the index: u32 index_offset |
 * u32 index_size | u32 0 | u32 0 | u32 crc32_, crc32_ the stamp of tkv_sst_stamp_footer.
 * file_size = index_offset + index_size + 20. All integers little-endian.
 * d_file may have any byte alignment; no byte outside [d_file, d_file + file_size) is written or
 * read-modify-written. *file_size, *n_blocks, *index_offset and *index_size are set whenever the
 * arguments are valid. file_size > cap, or n_blocks > block_cap with any block array non-NULL:
 * TKV_BUFFER_OVERFLOW with the four sizes set and nothing written to d_file or a block array (cap = 0
 * with d_file = NULL and NULL block arrays is the sizing call). Block arrays (device, each nullable,
 * block_cap entries): block_off[j] = O_j, block_size[j] = 36 + z_j, block_first[j] = b_j; the first two
 * are valid inputs of tkv_sst_block_crcs_device, and widened to u64 of tkv_sst_verify_blocks.
 * TKV_INVALID_ARGUMENT, decided before any byte is written and without reading a source byte, the four
 * sizes untouched: n == 0 (the reference writer verifies a non-empty block and index); n > 2^32 - 1;
 * target_block_size == 0; NULL where a pointer is required (keys, key_off, key_len, the four size
 * outputs; vals and val_off with val_len; d_file with cap > 0); some kl or vl >= 2^28 (its varint
 * would take 5 bytes where 4 are counted, and the body would overrun its counted size); some
 * 36 + z_j > 2^32 - 1 (the header fields are u32); file_size > 2^32 - 1 (the footer fields are u32).
 * The device call is synchronous on `stream` (the host needs the sizes before the emit); with no usable
 * GPU it returns TKV_IO_ERROR. No CRC is computed on the CPU and no image byte crosses PCIe. */
int tkv_sst_build_device(const uint8_t *d_keys, const uint64_t *d_key_off, const uint32_t *d_key_len,
                         const uint8_t *d_vals, const uint64_t *d_val_off, const uint32_t *d_val_len,
                         uint64_t n, uint32_t target_block_size,
                         uint8_t *d_file, uint64_t cap,
                         uint64_t *d_block_off, uint32_t *d_block_size, uint32_t *d_block_first, uint64_t block_cap,
                         uint64_t *file_size, uint64_t *n_blocks, uint64_t *index_offset, uint64_t *index_size,
                         void *stream);

/* The same with every pointer in HOST memory. The cut and the layout (CRC fields zero) are computed on
 * host threads; the stamps come from the paths tkv_sst_stamp_blocks and tkv_sst_stamp_footer use.
 * Sizing, overflow and argument errors are decided before any GPU call. */
int tkv_sst_build(const uint8_t *h_keys, const uint64_t *h_key_off, const uint32_t *h_key_len,
                  const uint8_t *h_vals, const uint64_t *h_val_off, const uint32_t *h_val_len,
                  uint64_t n, uint32_t target_block_size,
                  uint8_t *h_file, uint64_t cap,
                  uint64_t *h_block_off, uint32_t *h_block_size, uint32_t *h_block_first, uint64_t block_cap,
                  uint64_t *file_size, uint64_t *n_blocks, uint64_t *index_offset, uint64_t *index_size);

/* ---- SSTable scan: verify, index and entries of a file image in one call ---------- */

/* The reader of what tkv_sst_build[_device] writes, in the same columnar form: its outputs are valid
 * inputs of tkv_sst_build_device, its input is what that call writes. The reference leaves this half open
 * (decode_data_block_header and decode_data_block are stubs, sstable_reader::read_data_block returns an
 * empty block), so, like the stamps, what a reader checks is this library's decision, written down here.
 * Checks, in this order of precedence. All arithmetic is 64-bit; no byte outside [file, file + file_size)
 * is read, whatever the file holds; a length that failed a check is never used to copy or to walk.
 * Footer (else TKV_CORRUPTED with *bad_block = TKV_SST_BAD_FOOTER): 28 <= file_size <= 2^32 - 1; the last
 * 20 bytes are u32 index_offset | u32 index_size | u32 bloom_offset | u32 bloom_size | u32 crc32_ with
 * index_offset + index_size + 20 == file_size and index_size >= 8 (the bloom fields are not interpreted);
 * crc32_ equals the CRC-32 of [index_offset, index_offset + index_size + 16) (tkv_sst_verify_footer).
 * Index (else TKV_CORRUPTED, TKV_SST_BAD_INDEX): B = the u64 at the index start, B <= (index_size - 8) /
 * 17; then B entries varint(kl) | key | u64 off | u64 size, each length varint ending within 4 bytes
 * (value < 2^28; a redundant encoding such as 80 00 is taken at its value, as a LEB128 reader takes it),
 * each entry inside the index, size >= TKV_SST_MIN_IMAGE and off + size <= index_offset; the position
 * behind entry B - 1 is exactly index_size. B == 0 is a valid empty table: TKV_OK, all sizes 0. Blocks
 * need not tile the data region and may be listed in any order.
 * Block j, image [off_j, off_j + size_j): any failure makes block j bad and *bad_block is the smallest
 * bad j. Byte 0 is 0x14; c = the u32 at 1, z = the u32 at 5, the u32 at 9 equals z, byte 13 is 0 (the
 * three pad bytes are covered by the checksum only); 36 + z == size_j; c >= 1 and 8 c <= z; the varint
 * at byte 21 ends within 5 bytes and has the value z: the body is the z bytes behind it; the u32 at 17
 * equals the stamp (the CRC of the image with that field read as zero, tkv_sst_block_crcs_device's
 * value); the walk of c entries varint(kl) | key | varint(vl) | value from the body's start stays inside
 * the body, every varint ending within 4 bytes and inside the body; the sum of 8 + kl + vl over the c
 * entries equals z; the index entry's key equals the first entry's key, in length and bytes. Bytes
 * behind the last entry (slack and padding) are not inspected: the reference leaves arena bytes there.
 * Outputs, all in the index's order (block j's entries in front of block j + 1's): block_off / block_size
 * / block_first as tkv_sst_build_device's block arrays; key_len / val_len the lengths. Without a views
 * flag the spans are copied back to back into d_keys / d_vals, key_off / val_off are the exclusive u64
 * prefix sums of the lengths and *keys_size / *vals_size the totals. With a views flag nothing is copied
 * for that arena: the offsets point into the file image, the arena and its cap are ignored, the total is
 * still reported. Every output array is nullable and then skipped (a NULL arena is not written).
 * Destinations may have any byte alignment; nothing outside [d_keys, d_keys + *keys_size) and [d_vals,
 * d_vals + *vals_size) is written or read-modify-written.
 * TKV_CORRUPTED: *bad_block is set, the four sizes are 0, nothing is written to any output array.
 * TKV_OK: *bad_block = *n_blocks. TKV_BUFFER_OVERFLOW: the sizes are set and no array is written, when
 * *n_entries > entry_cap with any entry column non-NULL, *n_blocks > block_cap with any block array
 * non-NULL, or a copied arena's total is over its cap (all caps 0 with NULL arrays is the sizing call; it
 * returns TKV_OK for a table without a key or value byte). TKV_INVALID_ARGUMENT, decided before any
 * device work: NULL file with file_size > 0, unknown flag bits, NULL among the five scalar outputs,
 * file_size > 2^32 - 1. file_size < 28 is TKV_CORRUPTED with TKV_SST_BAD_FOOTER, not an argument error.
 * The device call is synchronous on `stream`; with no usable GPU it returns TKV_IO_ERROR; a scratch
 * allocation that fails returns TKV_OUT_OF_MEMORY (the scratch holds 24 bytes per index byte, 52 per block
 * and 40 per entry). No CRC is computed on the CPU and no file byte crosses PCIe: only a small pinned
 * result block does. */
#define TKV_SST_SCAN_KEY_VIEWS 1u   /* keys stay in the file image */
#define TKV_SST_SCAN_VAL_VIEWS 2u   /* values stay in the file image */
#define TKV_SST_BAD_FOOTER UINT64_MAX         /* *bad_block when the footer (or its checksum) fails */
#define TKV_SST_BAD_INDEX  (UINT64_MAX - 1)   /* *bad_block when the index framing fails */
int tkv_sst_scan_device(const uint8_t *d_file, uint64_t file_size, uint32_t flags,
                        uint64_t *d_key_off, uint32_t *d_key_len, uint64_t *d_val_off, uint32_t *d_val_len,
                        uint64_t entry_cap,
                        uint8_t *d_keys, uint64_t keys_cap, uint8_t *d_vals, uint64_t vals_cap,
                        uint64_t *d_block_off, uint32_t *d_block_size, uint32_t *d_block_first, uint64_t block_cap,
                        uint64_t *n_entries, uint64_t *n_blocks, uint64_t *keys_size, uint64_t *vals_size,
                        uint64_t *bad_block, void *stream);

/* The same contract for a host image, every pointer in HOST memory. Parsing and copies run on host
 * threads, one task per range of blocks; the checksums go through the paths tkv_sst_verify_footer and
 * tkv_sst_verify_blocks use. Argument errors and footer failures, apart from the footer's checksum, are
 * decided before any GPU call. */
int tkv_sst_scan(const uint8_t *h_file, uint64_t file_size, uint32_t flags,
                 uint64_t *h_key_off, uint32_t *h_key_len, uint64_t *h_val_off, uint32_t *h_val_len,
                 uint64_t entry_cap,
                 uint8_t *h_keys, uint64_t keys_cap, uint8_t *h_vals, uint64_t vals_cap,
                 uint64_t *h_block_off, uint32_t *h_block_size, uint32_t *h_block_first, uint64_t block_cap,
                 uint64_t *n_entries, uint64_t *n_blocks, uint64_t *keys_size, uint64_t *vals_size,
                 uint64_t *bad_block);

/* ---- Memtable replay: sort and dedupe a decoded WAL batch ------------------------- */

/* What a memtable holds after engine::create's replay loop (engine.cpp:30-47) has inserted a whole batch
 * (memtable.cpp:58-72, skiplist.hpp:201-242), in iteration order, for n records given in log order as the
 * columns tkv_wal_decode_device writes: user key K_i = [keys + key_off[i], + key_len[i]), value span
 * (val_off[i], val_len[i]), op[i], tomb[i], seq[i]. The outputs are valid inputs of tkv_sst_build_device.
 * Order: internal_key_comparator compares user keys only, through simd_comparator: unsigned bytewise, and
 * when one key is a prefix of the other the shorter is smaller ("" < "a" < "a\0" < "a\0\0" < "a\1" <
 * "\x80"). seq, tomb and op do not take part.
 * Replacement: skiplist::insert of an equal user key replaces the node, so of all records with one user
 * key the one LATEST IN INPUT ORDER survives, whatever its seq.
 * Operation: op == 0 (put) keeps the record's value span; op == 1 (del) stores an empty value (val_len 0,
 * val_off as the record's), whatever the record carried; any other op is the reference's FR_VERIFY abort:
 * TKV_CORRUPTED, *first_bad = the smallest such index, nothing written to any output array, *n_entries =
 * *ikeys_size = 0. tomb is taken from the record for both ops. Otherwise *first_bad = n.
 * Internal key (encode_internal_key, sstable_format.cpp:9-25): user_key | u64 seq LE | u64 timestamp LE |
 * u8 tombstone, 17 bytes behind the key. The tombstone byte is tomb[i] != 0. The reference's timestamp is
 * wall_clock_ms() at each put and cannot be reproduced: timestamp_ms goes into every internal key.
 * Inputs: val_off, val_len, op, tomb, seq are nullable (value spans (0, 0); every record a put; 0; 0).
 * VALUES ARE NEVER READ: there is no value arena among the arguments, and out_val_off / out_val_len are
 * spans in the arena the caller holds and passes on to tkv_sst_build_device as is. Key sources may have
 * any alignment, may overlap and may have gaps (the WAL image itself under TKV_WAL_DECODE_KEY_VIEWS); no
 * byte outside [keys, keys + keys_size) is read for any input, beyond the aligned 16-byte granule that
 * holds a key byte (the span copies of the WAL calls read the same way).
 * Outputs, each nullable and then skipped: m = *n_entries distinct keys, entry j the j-th smallest;
 * ikey_len[j] = key_len + 17, ikey_off[j] the exclusive u64 prefix sum of ikey_len, *ikeys_size the total;
 * the internal keys back to back in d_ikeys (any byte alignment; nothing outside [d_ikeys, d_ikeys +
 * *ikeys_size) is written or read-modify-written); out_val_off / out_val_len as above; src[j] = the index
 * of the surviving record. The result is unique (the sort is stable), so two calls agree byte for byte.
 * Sizing and overflow: m > entry_cap with any entry column non-NULL, or *ikeys_size > ikeys_cap with
 * d_ikeys non-NULL: TKV_BUFFER_OVERFLOW with both sizes set and nothing written (caps of 0 with NULL
 * arrays is the sizing call, TKV_OK).
 * TKV_INVALID_ARGUMENT, before any device work and with no output touched: n > 2^32 - 1; NULL n_entries /
 * ikeys_size / first_bad; with n > 0 NULL key_off / key_len, NULL keys with keys_size > 0, val_len without
 * val_off. Found by the check pass, again with no output touched and before an op is judged: some
 * key_off[i] + key_len[i] > keys_size; some key_len[i] + 17 >= 2^28 (the flush would refuse the entry).
 * More than 2^31 - 1 entries can be sized and listed but not written to d_ikeys.
 * n == 0: TKV_OK, sizes 0, *first_bad = 0, nothing else touched.
 * The device call is synchronous on `stream` (one host synchronisation per refinement round: at most
 * ceil(max key_len / 8) + 1 rounds, each over the still unresolved records only); with no usable GPU it
 * returns TKV_IO_ERROR; a scratch allocation that fails returns TKV_OUT_OF_MEMORY (the scratch holds 64
 * bytes per record, 40 more per entry when d_ikeys is written, 8 per 4 KiB of internal keys and 0.5 per
 * record for the histograms). No key byte crosses PCIe: only a small pinned result block does. */
int tkv_memtable_build_device(const uint8_t *d_keys, uint64_t keys_size,
                              const uint64_t *d_key_off, const uint32_t *d_key_len,
                              const uint64_t *d_val_off, const uint32_t *d_val_len,
                              const uint8_t *d_op, const uint8_t *d_tomb, const uint64_t *d_seq,
                              uint64_t n, uint64_t timestamp_ms,
                              uint8_t *d_ikeys, uint64_t ikeys_cap,
                              uint64_t *d_ikey_off, uint32_t *d_ikey_len,
                              uint64_t *d_out_val_off, uint32_t *d_out_val_len, uint32_t *d_src,
                              uint64_t entry_cap,
                              uint64_t *n_entries, uint64_t *ikeys_size, uint64_t *first_bad, void *stream);

/* The same contract with every pointer in HOST memory: a stable sort of record indices with a full-key
 * comparator on host threads (chunk sorts, then pairwise merges), then the same dedupe and emit. It uses
 * no GPU at all and is NOT a fallback of the device call. */
int tkv_memtable_build(const uint8_t *h_keys, uint64_t keys_size,
                       const uint64_t *h_key_off, const uint32_t *h_key_len,
                       const uint64_t *h_val_off, const uint32_t *h_val_len,
                       const uint8_t *h_op, const uint8_t *h_tomb, const uint64_t *h_seq,
                       uint64_t n, uint64_t timestamp_ms,
                       uint8_t *h_ikeys, uint64_t ikeys_cap,
                       uint64_t *h_ikey_off, uint32_t *h_ikey_len,
                       uint64_t *h_out_val_off, uint32_t *h_out_val_len, uint32_t *h_src,
                       uint64_t entry_cap,
                       uint64_t *n_entries, uint64_t *ikeys_size, uint64_t *first_bad);

/* ---- SSTable merge: k-way merge of sorted runs, newest wins ----------------------- */

#define TKV_SST_MERGE_DROP_TOMBSTONES 1u   /* a surviving tombstone is left out (the last level) */
#define TKV_SST_MERGE_MAX_RUNS 64u
#define TKV_SST_MERGE_NONE UINT64_MAX      /* *first_bad when nothing is bad */

/* Compaction's merge: n_runs sorted runs of internal keys into one run without shadowed entries. The
 * per-run arguments (d_keys, keys_size, d_key_off, d_key_len, d_val_off, d_val_len, n, val_bias) are HOST
 * arrays of n_runs elements; the elements of the pointer arrays are device pointers (host pointers for
 * tkv_sst_merge).
 * Runs are given OLDEST FIRST. Run r holds n[r] entries; entry i has the internal key [d_keys[r] +
 * key_off_r[i], + key_len_r[i]) and the value span (val_off_r[i], val_len_r[i]): exactly the columns
 * tkv_sst_scan_device returns with both view flags, and the ones tkv_memtable_build_device returns.
 * d_val_off / d_val_len may be NULL as a whole or per run: every value of that run is then empty, span
 * (0, 0) plus the bias. VALUES ARE NEVER READ; keys are read but never copied.
 * Keys: the user key of an entry is its internal key without the last 17 bytes (u64 seq | u64 timestamp |
 * u8 tombstone). Sequence and timestamp are NOT interpreted. The tombstone is the last byte, != 0.
 * Order: the memtable replay's: user keys as unsigned bytes, a prefix first. Each run must be ascending by
 * user key, non-strictly: equal neighbours inside one run are allowed.
 * Survivor: of all entries with one user key the one from the HIGHEST-NUMBERED RUN survives, and within
 * that run the one with the highest index: the replay's "latest in input order" applied to the
 * concatenation of the runs. It is NOT "highest sequence": skiplist::insert replaces the node of an equal
 * user key whatever its seq (skiplist.hpp:201-242), so the entry written last is the one a reader of the
 * reference would find, and a merge that looked at seq would disagree with the replay on the same records.
 * Tombstone drop: with TKV_SST_MERGE_DROP_TOMBSTONES a survivor whose tombstone byte is non-zero is left
 * out; it still shadows the older entries of its key. Without the flag it is kept with its value span as
 * given.
 * Outputs, each nullable and then skipped: the m = *n_entries survivors ascending; out_key_len[j] /
 * out_val_len[j] copied; out_key_off[j] = (d_keys[r] - d_key_base) + key_off_r[i]; out_val_off[j] =
 * val_bias[r] + val_off_r[i] (val_bias NULL: zeros); out_src[j] = r << 32 | i; *keys_bytes / *vals_bytes
 * the sums of the survivors' lengths. The offsets are meant for the flush, tkv_sst_build_device with
 * d_key_base, out_key_off, out_key_len, the value base, out_val_off, out_val_len and m: that call takes one
 * base per arena and has no arena size. The result is unique, so two calls agree bit for bit.
 * Sizing and overflow: m > entry_cap with any output column non-NULL: TKV_BUFFER_OVERFLOW with the three
 * sizes set and nothing written (entry_cap 0 with all columns NULL is the sizing call, TKV_OK).
 * TKV_CORRUPTED, found by a check pass (on the device in the device call), no output array written, the
 * three sizes 0: *first_bad = the smallest r << 32 | i for which key_len < 17, or key_len >= 2^28, or
 * key_off + key_len > keys_size[r], or entries i and i - 1 both pass these three checks and the user key of
 * i is smaller than that of i - 1. Otherwise *first_bad = TKV_SST_MERGE_NONE.
 * TKV_INVALID_ARGUMENT, before any device work and with nothing touched: n_runs > TKV_SST_MERGE_MAX_RUNS;
 * unknown flag bits; NULL n_entries / keys_bytes / vals_bytes / first_bad; with n_runs > 0 NULL d_keys /
 * keys_size / d_key_off / d_key_len / n, or a NULL element of d_keys / d_key_off / d_key_len for a run
 * with n[r] > 0; d_val_len[r] without d_val_off[r]; some n[r] > 2^32 - 1 or the total N > 2^32 - 1;
 * d_key_base NULL or above some d_keys[r] of a non-empty run while d_out_key_off is non-NULL.
 * n_runs == 0 or N == 0: TKV_OK, sizes 0, *first_bad = TKV_SST_MERGE_NONE, nothing else touched. Empty
 * runs among non-empty ones are fine.
 * Reads: no byte outside [d_keys[r], d_keys[r] + keys_size[r]) is read, beyond the aligned 16-byte granule
 * that holds a key byte (the replay's rule).
 * The device call is synchronous on `stream` with TWO host synchronisations, whatever K, N and the key
 * lengths: one for the verdict and the sizes (the kernels behind the check pass read the verdict on the
 * device and do nothing on bad input, so the host need not wait in between), one at the end of the emit.
 * With no usable GPU it returns TKV_IO_ERROR; a scratch allocation that fails returns TKV_OUT_OF_MEMORY
 * (the scratch holds 41 bytes per input entry: two lists of 16-byte sort entries, the survivor scan and
 * a flag; plus 16 bytes per workgroup tile of every round and 24 per 1024 entries for the scan's sums). No key byte crosses PCIe: only the run table,
 * the tile map and a small pinned result block do. One GPU; K > 64 is refused. */
int tkv_sst_merge_device(uint32_t n_runs,
                         const uint8_t *const *d_keys, const uint64_t *keys_size,
                         const uint64_t *const *d_key_off, const uint32_t *const *d_key_len,
                         const uint64_t *const *d_val_off, const uint32_t *const *d_val_len,
                         const uint64_t *n,
                         const uint8_t *d_key_base, const uint64_t *val_bias, uint32_t flags,
                         uint64_t *d_out_key_off, uint32_t *d_out_key_len,
                         uint64_t *d_out_val_off, uint32_t *d_out_val_len, uint64_t *d_out_src,
                         uint64_t entry_cap,
                         uint64_t *n_entries, uint64_t *keys_bytes, uint64_t *vals_bytes, uint64_t *first_bad,
                         void *stream);

/* The same contract with every pointer in HOST memory: the runs validated on host threads, then
 * neighbouring lists merged pairwise on host threads with a full-key comparator (the older side first on
 * equal keys), then the same survivor rule and emit. It uses no GPU at all and is NOT a fallback of the
 * device call. */
int tkv_sst_merge(uint32_t n_runs,
                  const uint8_t *const *h_keys, const uint64_t *keys_size,
                  const uint64_t *const *h_key_off, const uint32_t *const *h_key_len,
                  const uint64_t *const *h_val_off, const uint32_t *const *h_val_len,
                  const uint64_t *n,
                  const uint8_t *h_key_base, const uint64_t *val_bias, uint32_t flags,
                  uint64_t *h_out_key_off, uint32_t *h_out_key_len,
                  uint64_t *h_out_val_off, uint32_t *h_out_val_len, uint64_t *h_out_src,
                  uint64_t entry_cap,
                  uint64_t *n_entries, uint64_t *keys_bytes, uint64_t *vals_bytes, uint64_t *first_bad);

/* ---- SSTable get: batched point lookup over sorted runs, newest wins --------------- */

#define TKV_SST_GET_ABSENT  0u   /* no run holds the user key */
#define TKV_SST_GET_FOUND   1u   /* the newest entry of the key is live */
#define TKV_SST_GET_DELETED 2u   /* the newest entry of the key is a tombstone */

/* engine::get for a batch: nq user keys looked up in n_runs sorted runs of internal keys, the memtable runs
 * behind the segments' (engine.cpp:91-121 walks the memtables, then segments_; segment::get_kv_entry does
 * not compile in the reference, so the read contract is fixed here).
 * The per-run arguments (d_keys, keys_size, d_key_off, d_key_len, d_val_off, d_val_len, n, d_vals,
 * vals_size, val_bias) are tkv_sst_merge_device's, with the same meaning: HOST arrays of n_runs elements
 * whose pointer elements are device pointers (host pointers for tkv_sst_get), runs OLDEST FIRST, n_runs <=
 * TKV_SST_MERGE_MAX_RUNS, d_val_off / d_val_len NULL as a whole or per run (every value of that run is
 * empty). d_vals[r] / vals_size[r] name run r's value arena: val_off_r counts from d_vals[r].
 * Queries: user key j is [d_qkeys + q_off[j], + q_len[j]). The user key of an entry is its internal key
 * without the last 17 bytes; order is the replay's (unsigned bytes, a prefix first).
 * Lookup rule: for query j the runs are visited from the HIGHEST-NUMBERED one down. In a run the hit is the
 * entry with the highest index whose user key equals the query (the upper bound minus one). The first run
 * with a hit decides: TKV_SST_GET_FOUND when the hit's last key byte is 0, else TKV_SST_GET_DELETED; older
 * runs are not consulted (engine.cpp:110-118 stops at a tombstone). No hit anywhere: TKV_SST_GET_ABSENT.
 * Sequence and timestamp take no part. The answer is the one a lookup in tkv_sst_merge_device's output
 * without the drop flag gives.
 * Per-query outputs, each nullable and then skipped: state[j]; src[j] = r << 32 | i of the hit,
 * TKV_SST_MERGE_NONE when ABSENT; seq[j] = the u64 behind the hit's user key, 0 when ABSENT;
 * out_val_off[j] = val_bias[r] + val_off_r[i] (val_bias NULL: zeros) and out_val_len[j] = val_len_r[i] for
 * FOUND, (0, 0) otherwise: a DELETED hit reports no value, whatever the entry carries. *n_found = the
 * count of FOUND.
 * Value gather: d_vals non-NULL switches it on. The values of the FOUND queries are copied back to back, in
 * query order, into d_out_vals; out_val_pos[j] = the exclusive u64 prefix sum of out_val_len; *vals_bytes
 * = the total, reported without the gather too. *vals_bytes > vals_cap with d_out_vals non-NULL:
 * TKV_BUFFER_OVERFLOW with the two sizes set and nothing written (all outputs NULL and vals_cap 0 is the
 * sizing call, TKV_OK). Many queries may hit one entry: its value is copied once per query. d_out_vals may
 * have any byte alignment; nothing outside [d_out_vals, + *vals_bytes) is written or read-modify-written.
 * THE RUNS ARE NOT VALIDATED AS A WHOLE (a pass over N entries per call would defeat the purpose): they
 * must be ascending, as the scan, the replay and the merge return them; on a run that is not, the answers
 * are unspecified but the call stays memory-safe. The search of a run of n entries is fixed: pos = 0; for
 * step = 2^(b - 1), ..., 2, 1 with b = ceil(log2(n + 1)): entry pos + step - 1 is probed when pos + step
 * <= n, and pos += step when its user key is <= the query; the hit is entry pos - 1 when the last probe
 * that advanced pos compared equal. Every probed entry is span-checked before its key is read (key_len >=
 * 17, key_len < 2^28, key_off + key_len <= keys_size[r]); with the gather on, a FOUND hit's val_off +
 * val_len <= vals_size[r] is checked too (a NULL d_vals[r] counts as an arena of 0 bytes). A query stops at
 * its first failed check. Any failed check: TKV_CORRUPTED, *first_bad = the smallest r << 32 | i among the
 * entries that were read and failed (the probe sequence is the one above in both calls, so this is
 * deterministic), the two sizes 0, no output array written. An entry no search reads is not checked.
 * Otherwise *first_bad = TKV_SST_MERGE_NONE.
 * Bad queries: q_off[j] + q_len[j] > qkeys_size or q_len[j] + 17 >= 2^28 for some j: TKV_INVALID_ARGUMENT,
 * found by the first pass (on the device in the device call), no output touched. It goes before
 * TKV_CORRUPTED.
 * TKV_INVALID_ARGUMENT, before any device work and with nothing touched: the merge's errors for the run
 * arguments (n_runs > TKV_SST_MERGE_MAX_RUNS; with n_runs > 0 NULL d_keys / keys_size / d_key_off /
 * d_key_len / n, or a NULL element of d_keys / d_key_off / d_key_len for a run with n[r] > 0; d_val_len[r]
 * without d_val_off[r]; some n[r] > 2^32 - 1 or the total N > 2^32 - 1); flags != 0; NULL n_found /
 * vals_bytes / first_bad; with nq > 0 NULL d_q_off / d_q_len, or NULL d_qkeys with qkeys_size > 0; nq >
 * 2^32 - 1; d_vals without vals_size; d_out_vals or d_out_val_pos without d_vals.
 * nq == 0: TKV_OK, sizes 0, *first_bad = TKV_SST_MERGE_NONE, nothing else touched. n_runs == 0 or every
 * run empty: every query is ABSENT.
 * Reads: no byte outside a run's [d_keys[r], + keys_size[r]) or [d_qkeys, + qkeys_size) is read, beyond the
 * aligned 16-byte granule that holds a key byte (the replay's rule); values are read only by the gather,
 * and only inside [d_vals[r], + vals_size[r]) under the same rule.
 * The device call is synchronous on `stream` with at most TWO host synchronisations: one for the verdicts
 * and the sizes (the kernels behind the search read the verdicts on the device and write nothing when one
 * is set), one at the end of the emit. With no usable GPU it returns TKV_IO_ERROR; a scratch allocation
 * that fails returns TKV_OUT_OF_MEMORY (the scratch holds 32 bytes per query: the hit, state and value
 * length, and the two scans; plus 16 bytes per 1024 queries for the scans' sums, 8 per 4096 gathered bytes
 * for the emit's tile table and 96 per run). No key byte crosses PCIe: only the run table and a small
 * pinned result block do. One GPU. */
int tkv_sst_get_device(uint32_t n_runs,
                       const uint8_t *const *d_keys, const uint64_t *keys_size,
                       const uint64_t *const *d_key_off, const uint32_t *const *d_key_len,
                       const uint64_t *const *d_val_off, const uint32_t *const *d_val_len,
                       const uint64_t *n,
                       const uint8_t *const *d_vals, const uint64_t *vals_size,   /* nullable: no gather */
                       const uint64_t *val_bias,
                       const uint8_t *d_qkeys, uint64_t qkeys_size,
                       const uint64_t *d_q_off, const uint32_t *d_q_len, uint64_t nq, uint32_t flags,
                       uint8_t *d_state, uint64_t *d_src, uint64_t *d_seq,
                       uint64_t *d_out_val_off, uint32_t *d_out_val_len,
                       uint64_t *d_out_val_pos, uint8_t *d_out_vals, uint64_t vals_cap,
                       uint64_t *n_found, uint64_t *vals_bytes, uint64_t *first_bad, void *stream);

/* The same contract with every pointer in HOST memory: the queries split over host threads, the same
 * search with a full-key comparator, the same checks on probed entries only, the same verdict precedence
 * and outputs. It uses no GPU at all and is NOT a fallback of the device call. */
int tkv_sst_get(uint32_t n_runs,
                const uint8_t *const *h_keys, const uint64_t *keys_size,
                const uint64_t *const *h_key_off, const uint32_t *const *h_key_len,
                const uint64_t *const *h_val_off, const uint32_t *const *h_val_len,
                const uint64_t *n,
                const uint8_t *const *h_vals, const uint64_t *vals_size,
                const uint64_t *val_bias,
                const uint8_t *h_qkeys, uint64_t qkeys_size,
                const uint64_t *h_q_off, const uint32_t *h_q_len, uint64_t nq, uint32_t flags,
                uint8_t *h_state, uint64_t *h_src, uint64_t *h_seq,
                uint64_t *h_out_val_off, uint32_t *h_out_val_len,
                uint64_t *h_out_val_pos, uint8_t *h_out_vals, uint64_t vals_cap,
                uint64_t *n_found, uint64_t *vals_bytes, uint64_t *first_bad);

/* ---- CRC-32C (Castagnoli) — SURVEY.md §8f rank 4 ------------------------------------------------ */

/* Same engine and kernels with the tables of the Castagnoli polynomial (reflected 0x82F63B78,
 * init/xorout 0xFFFFFFFF: iSCSI, RFC 3720 §B.4). Not reference behaviour; offered for a
 * format-versioned alternative. Arguments and conventions as for the tkv_crc32_* functions. */
#define TKV_CRC32C_POLYNOMIAL 0x82F63B78u
int tkv_crc32c_update(uint32_t raw_state, const void *data, size_t len, uint32_t *out_raw);
int tkv_crc32c_update_device(uint32_t raw_state, const void *d_data, size_t len, uint32_t *d_out_raw,
                             void *stream);
int tkv_crc32c_batch_device(const uint8_t *d_base, const uint64_t *d_offsets, const uint32_t *d_lengths,
                            const uint32_t *d_init_raw, uint32_t *d_out_final, uint64_t n, void *stream);
int tkv_crc32c_batch_uniform_device(const uint8_t *d_base, uint64_t stride, uint64_t len,
                                    const uint32_t *d_init_raw, uint32_t *d_out_final, uint64_t n,
                                    void *stream);
int tkv_crc32c_batch_host(const uint8_t *h_base, const uint64_t *h_offsets, const uint32_t *h_lengths,
                          const uint32_t *h_init_raw, uint32_t *h_out_final, uint64_t n);
int tkv_crc32c_batch_host_multi(const int *devices, int ndev, const uint8_t *h_base, const uint64_t *h_offsets,
                                const uint32_t *h_lengths, const uint32_t *h_init_raw, uint32_t *h_out_final,
                                uint64_t n);
uint32_t tkv_crc32c_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* ---- synthetic data (SURVEY.md §8d generator; bench/test inputs) ------------------------------- */

int tkv_fill_synthetic_uniform(uint8_t *d_dst, uint64_t stride, uint64_t len, uint64_t first_block,
                               uint64_t nblocks, uint64_t seed, void *stream);
int tkv_fill_synthetic_blocks(uint8_t *d_base, const uint64_t *d_offsets, const uint32_t *d_lengths,
                              uint64_t first_block, uint64_t nblocks, uint64_t seed, void *stream);

/* ---- introspection for tests (no GPU needed) --------------------------------------------------- */

/* Copy the constant tables the kernels use (layout of tkv::DeviceTables) into `out`; returns the
 * byte size needed (call with out = NULL to query). */
size_t tkv_debug_tables(void *out, size_t cap);
/* Same for any reflected polynomial (TKV_CRC32_POLYNOMIAL, TKV_CRC32C_POLYNOMIAL). */
size_t tkv_debug_tables_poly(uint32_t poly, void *out, size_t cap);

/* Host GF(2) helpers the decomposition rests on: a*b mod P and x^(8n) mod P, reflected. */
uint32_t tkv_debug_multmodp(uint32_t a, uint32_t b);
/* The record chain tkv_wal_verify walks (host only, no CRC): writes up to `cap` record start offsets,
 * the offset after the last record and whether a header did not fit; returns the record count. */
size_t tkv_debug_wal_chain(const uint8_t *h_wal, uint64_t size, uint64_t *out_pos, size_t cap, uint64_t *end,
                           int *err);
uint32_t tkv_debug_x8nmodp(uint64_t nbytes);
/* The split tkv_crc32_batch_host_multi plans for `ndev` devices (host only, no device, no CRC):
 * writes up to `cap` pieces as 6 x u64 records {device, block, byte offset, length, initial raw
 * register, starts its block} in device order, pieces in block order; returns the piece count. */
size_t tkv_debug_multi_plan(int ndev, const uint64_t *h_offsets, const uint32_t *h_lengths,
                            const uint32_t *h_init_raw, uint64_t n, uint64_t *out_rec, size_t cap);
/* The host combine step of that plan: given each piece's finalized CRC (in the order
 * tkv_debug_multi_plan lists them), writes every block's finalized CRC. 4-byte GF(2) arithmetic on
 * registers only, for the reflected polynomial `poly`. */
int tkv_debug_multi_combine(uint32_t poly, int ndev, const uint64_t *h_offsets, const uint32_t *h_lengths,
                            const uint32_t *h_init_raw, uint64_t n, const uint32_t *piece_final,
                            uint32_t *h_out_final);
/* Update calls of the calling thread so far: out[0] through tkv_crc32[c]_update_host (the drop-in's
 * short-span host path), out[1] through tkv_crc32[c]_update (the GPU). (The round-3 entry point:
 * two words.) */
void tkv_debug_update_counts(uint64_t out[2]);
/* The same counters into out[0..n) (n may be smaller or larger than the count), plus out[2] = calls
 * through tkv_crc32[c]_update_fallback (host recomputes after a failed GPU update). Returns the number
 * of counters (3). */
size_t tkv_debug_update_counts_n(uint64_t *out, size_t n);
/* What the calling thread's last tkv_wal_verify / tkv_wal_verify_device did: out[0] = device
 * rounds (the sweep, then one per fix-up round), out[1] = 1 when it handed the image to the exact
 * host-thread walk (only a host image the device cannot hold), out[2] = 1 when a host image was
 * copied to the device, out[3] = 1 when the sweep needed no fix-up (0 when no device round ran). */
void tkv_debug_wal_last(uint64_t out[4]);
/* Per fix-up round of the calling thread's last device WAL verify, six words each: failing chunk
 * boundaries found, fix-up tasks launched, the longest task's range and all tasks' ranges (regions a
 * task may walk), the most regions one task walked and all regions walked. Writes up to n words;
 * returns the number available (0 when the sweep needed no fix-up). */
size_t tkv_debug_wal_rounds(uint64_t *out, size_t n);
/* Fix-up rounds a device WAL verify or index may take before it hands the image to the exact host walk
 * (default 256; 0 restores it). Returns the previous value. Tests set 1 to reach the hand-over. */
uint64_t tkv_debug_set_wal_round_budget(uint64_t rounds);
/* A cap on the waves of the device WAL sweep: a verify, index, salvage or recovery of nreg regions runs
 * min(nreg, 12 waves per compute unit, waves) of them, each over a contiguous chunk of regions (0: no
 * cap, the default). Process-wide, read once per sweep. Returns the previous value. Tests set 1-5 so
 * that images of a few regions run chunks of several regions, as images of tens of MB do. */
uint32_t tkv_debug_set_wal_sweep_waves(uint32_t waves);
/* Geometry of the device WAL sweep: out[0] = image bytes per region, out[1] = bytes per lane piece of
 * a region, out[2] = the waves of the calling thread's last sweep, out[3] = its regions (both 0 before
 * the first). */
void tkv_debug_wal_sweep_geometry(uint64_t out[4]);
/* Which path the last irregular batch on `stream` took: 1 = byte-stream row walk (blocks back to
 * back, each at least 64 bytes), 0 = general row walk; -1 on error. Synchronizes
 * the stream. */
int tkv_debug_irregular_mode(void *stream);
/* Which of crc_stream's general-path phases the last irregular batch on `stream` ran (0 in stream
 * mode): bit 0 the lane phase (blocks <= 64 B), bits 1 / 2 the 4- / 8-lane group passes (65-256 /
 * 257-512 B); -1 on error. Synchronizes the stream. */
int tkv_debug_irregular_phases(void *stream);
/* Which path folded the last irregular batch on `stream`: 0 = the one-pass kernel with one lane per
 * block only (crc_list_lanes: every block <= 64 B), 1 = the one-pass kernel with its packed mode in
 * at least one wave (every block <= 1 KiB), 2 = the general path after the one-pass kernel handed the
 * batch on (a block over 1 KiB), 3 = the general path alone (fewer than 256 K blocks, per-block
 * initial registers, tkv_debug_set_one_pass(0) or tkv_debug_set_stream_groups(1)); -1 on error.
 * Synchronizes the stream. */
int tkv_debug_irregular_path(void *stream);
/* Waves of the one-pass lane kernel (crc_list_lanes) for an irregular batch of nblocks on the current
 * device: wave w takes its 64-block steps [w TS / W, (w + 1) TS / W), TS = ceil(nblocks / 64). 0 when
 * no device is usable. */
uint32_t tkv_debug_list_lanes_waves(uint64_t nblocks);
/* The small-block lists of the last irregular batch on `stream` (all 0 in stream mode): out[0] =
 * blocks of at most 1 KiB the small-block phase folds (those no lane or group pass took), out[1] =
 * how many of them are at most 256 bytes (4-lane groups), out[2] = 257-512 bytes (8-lane groups; the
 * rest take 16-lane groups). Returns 0, or -1 on error. Synchronizes the stream. */
int tkv_debug_irregular_lists(void *stream, uint32_t out[3]);
/* Host batches from pinned host memory are read in place by the kernels (zero copy) unless this is
 * 0 (then they take the staged copy pipeline, as pageable memory does). Returns the previous
 * setting. Default 1; the environment variable TKV_HOST_MAPPED=0 sets 0 at load time. */
int tkv_debug_set_host_mapped(int enable);
/* Back-to-back irregular batches with a 4096-block scan tile of at least 1024 blocks of at most
 * 1 KiB and at most 1024 rows (4 MiB) of larger blocks take the general path, whose group passes and
 * small phase fold those blocks, unless this is 1: then they may take the byte-stream
 * walk as before round 4 (kept so its many-ends-per-row shapes stay under test). Returns the previous
 * setting. Default 0. */
int tkv_debug_set_stream_groups(int enable);
/* Irregular batches of at least 256 K blocks with the default register start with the one-pass
 * kernel (crc_list_lanes and its packed mode) unless this is 0: then they take the general path alone, as
 * smaller batches do (kept so the general path's large-batch shapes stay under test). Returns the
 * previous setting. Default 1. */
int tkv_debug_set_one_pass(int enable);
/* Packed uniform CRC-32 batches (blocks a multiple of 4 KiB, back to back, 16-byte aligned) fold 24 of
 * every lane's 64 bytes away with shifts and XORs modulo a sparse multiple of the polynomial before
 * the table steps unless this is 0: then they take the table-only kernel, as CRC-32C
 * always does (kept so one process can run both on the same buffers). Returns the previous setting.
 * Default 1. */
int tkv_debug_set_packed_fold(int enable);
/* Packed uniform batches of 4 KiB blocks. Each returns the previous setting; both are
 * kept so one process can run old and new on the same buffers, and every setting gives the same CRCs.
 * window: result registers (64 results each) a wave keeps before it stores any, 0..4 (other values are
 * clamped); 0 stores each register as soon as it is full. Default 4.
 * order: the waves take the batch's whole rounds of 16 x waves blocks in chunks of 16 consecutive blocks,
 * wave w chunks w, w + waves, ..., and share the rest evenly, unless this is 0: then every wave takes one
 * contiguous range of blocks. Default 1. */
int tkv_debug_set_packed_window(int registers);
int tkv_debug_set_packed_order(int enable);
/* tkv_crc32_batch_uniform_device with every block starting from the raw register init_raw instead of
 * 0xFFFFFFFF (the uniform kernels take any such register; the public entries only pass it for single
 * spans, so this keeps it under test on batches). */
int tkv_debug_batch_uniform_init_device(const uint8_t *d_base, uint64_t stride, uint64_t len, uint32_t init_raw,
                                        uint32_t *d_out_final, uint64_t n, void *stream);
/* The host layout step of tkv_wal_encode alone (no GPU): the records with their CRC fields zero, what
 * wal.cpp:27-52 leaves before line 54. Arguments as tkv_wal_encode; returns the number of records laid
 * out (0 on an argument error or when total > cap) and sets *img_size as tkv_wal_encode does. */
size_t tkv_debug_wal_encode_layout(const uint8_t *h_keys, const uint64_t *h_key_off, const uint32_t *h_key_len,
                                   const uint8_t *h_vals, const uint64_t *h_val_off, const uint32_t *h_val_len,
                                   const uint8_t *h_op, const uint8_t *h_tomb, const uint64_t *h_seq,
                                   uint64_t first_seq, uint64_t n, uint8_t *h_img, uint64_t cap,
                                   uint64_t *img_size);
/* Geometry of tkv_wal_encode_device: out[0] = image bytes per emit tile, out[1] = records per
 * workgroup of the size scan, out[2] = the largest record_len that is always stamped inside the emit
 * pass, out[3] = number of scan levels (for 2^32 - 1 records). */
void tkv_debug_wal_encode_geometry(uint64_t out[4]);
/* What the calling thread's last tkv_wal_encode_device did: out[0] = records stamped inside the emit
 * pass, out[1] = records stamped by reading the written image back, out[2] = emit waves, out[3] = total
 * bytes (all 0 when it wrote nothing). */
void tkv_debug_wal_encode_last(uint64_t out[4]);
/* tkv_wal_encode_device stamps records of record_len <= 240 inside its emit pass unless this is 0:
 * then every record is stamped by the read-back route (kept so one process can run both routes on the
 * same inputs). Returns the previous setting. Default 1. */
int tkv_debug_set_wal_encode_fused(int enable);
/* Geometry of tkv_wal_decode_device: out[0] = arena bytes per emit tile, out[1] = records per workgroup
 * of the length scans, out[2] = the longest span one lane copies (longer ones are copied by the whole
 * wave), out[3] = number of scan levels (for 2^32 - 1 records). */
void tkv_debug_wal_decode_geometry(uint64_t out[4]);
/* What the calling thread's last tkv_wal_decode_device did: out[0] = emit waves for the key arena,
 * out[1] = emit waves for the value arena (0 for a views or empty arena), out[2] = key bytes, out[3] =
 * value bytes (all 0 when it wrote nothing). */
void tkv_debug_wal_decode_last(uint64_t out[4]);
/* Geometry of tkv_wal_resync_device's search: out[0] = start offsets one wave tests per window, out[1] =
 * start offsets of a search's first span, out[2] = of its largest (spans grow fourfold in between),
 * out[3] = the one fixed-size hand-over of the search: the long candidates (record_len above 64 KiB) in
 * front of a batch's first valid short one that are folded one by one; a batch with more of them, which
 * one window can hold, takes the overflow route, a second run of the batch engine over its list. Short
 * candidates have no such limit: the survivor masks hold every density. */
void tkv_debug_wal_salvage_geometry(uint64_t out[4]);
/* What the calling thread's last tkv_wal_resync_device or tkv_wal_salvage[_device] did: out[0] =
 * resynchronisations, out[1] = search spans launched, out[2] = start offsets tested, out[3] = candidates
 * whose CRC was computed, out[4] = payload bytes folded for them, out[5] = index calls. */
void tkv_debug_wal_salvage_last(uint64_t out[6]);
/* The cut and the layout of tkv_sst_build alone (host only, no GPU): the file image with every CRC
 * field zero, the sizes and the block arrays. Arguments, status codes and what is left untouched on an
 * error are tkv_sst_build's. */
int tkv_debug_sst_build_layout(const uint8_t *h_keys, const uint64_t *h_key_off, const uint32_t *h_key_len,
                               const uint8_t *h_vals, const uint64_t *h_val_off, const uint32_t *h_val_len,
                               uint64_t n, uint32_t target_block_size, uint8_t *h_file, uint64_t cap,
                               uint64_t *h_block_off, uint32_t *h_block_size, uint32_t *h_block_first,
                               uint64_t block_cap, uint64_t *file_size, uint64_t *n_blocks, uint64_t *index_offset,
                               uint64_t *index_size);
/* Geometry of tkv_sst_build_device: out[0] = file bytes per emit tile, out[1] = entries per workgroup of
 * the scans, out[2] = entries whose hops the block cut composes in LDS before the doubling rounds (0:
 * plain doubling over the entries), out[3] = 0. */
void tkv_debug_sst_build_geometry(uint64_t out[4]);
/* What the calling thread's last tkv_sst_build_device did: out[0] = data blocks, out[1] = doubling
 * rounds of the block cut, out[2] = emit waves, out[3] = file bytes (all 0 when it wrote nothing). */
void tkv_debug_sst_build_last(uint64_t out[4]);
/* Phase times of the calling thread's last tkv_sst_build_device, in milliseconds between device events
 * on its stream: out_ms[0] = size scans, out_ms[1] = block cut and index layout (with the host's read of
 * the scan result in front), out_ms[2] = positions, tiles, emit and index (with the host's read of the
 * cut's result in front), out_ms[3] = CRC batch and stamp. All 0 unless timing was enabled before that
 * call. `enable` switches the timing of this thread's later calls on or off (default off: no events are
 * created); returns the previous setting. out_ms may be NULL. */
int tkv_debug_sst_build_phases(int enable, double out_ms[4]);
/* tkv_sst_scan with every checksum comparison skipped (host only, no GPU): the parse and the copies
 * alone, the counterpart of tkv_debug_sst_build_layout. Arguments, status codes and what is left
 * untouched on an error are tkv_sst_scan's. */
int tkv_debug_sst_scan_parse(const uint8_t *h_file, uint64_t file_size, uint32_t flags,
                             uint64_t *h_key_off, uint32_t *h_key_len, uint64_t *h_val_off, uint32_t *h_val_len,
                             uint64_t entry_cap,
                             uint8_t *h_keys, uint64_t keys_cap, uint8_t *h_vals, uint64_t vals_cap,
                             uint64_t *h_block_off, uint32_t *h_block_size, uint32_t *h_block_first,
                             uint64_t block_cap,
                             uint64_t *n_entries, uint64_t *n_blocks, uint64_t *keys_size, uint64_t *vals_size,
                             uint64_t *bad_block);
/* Geometry of tkv_sst_scan_device: out[0] = body bytes a parse window is walked for, out[1] = bytes of
 * varint look-ahead behind them, out[2] = arena bytes per emit tile, out[3] = entries per workgroup of the
 * scans. */
void tkv_debug_sst_scan_geometry(uint64_t out[4]);
/* What the calling thread's last tkv_sst_scan_device did: out[0] = data blocks, out[1] = doubling rounds
 * of the index chain, out[2] = parse waves, out[3] = emit waves of both arenas (all 0 when it did not
 * reach its end). */
void tkv_debug_sst_scan_last(uint64_t out[4]);
/* Phase times of the calling thread's last tkv_sst_scan_device that returned TKV_OK, in milliseconds
 * between device events on its stream: out_ms[0] = open (footer fields, index chain, ranks, block list,
 * with the host's read of the footer in front), out_ms[1] = checksum (the CRC batch and the comparison),
 * out_ms[2] = parse (both passes and the count scan, with the host's read of the verdict between them),
 * out_ms[3] = emit (length scans, columns, arena gathers). Switch and return value as
 * tkv_debug_sst_build_phases. */
int tkv_debug_sst_scan_phases(int enable, double out_ms[4]);

/* Geometry of tkv_memtable_build_device: out[0] = entries per workgroup of a radix pass, out[1] = buckets
 * of a pass, out[2] = passes a round runs at most (4 digit bits, 8 word bytes, 4 segment bytes; a pass
 * whose bits are the same in every entry is skipped), out[3] = internal-key bytes per emit tile. A list
 * of up to out[0] entries is sorted by one workgroup per pass, a longer one by histogram, scan and
 * scatter. */
void tkv_debug_memtable_geom(uint64_t out[4]);
/* What the calling thread's last tkv_memtable_build_device did: out[0] = survivors, out[1] = refinement
 * rounds run (the first sort included), out[2] = records that entered the second round (longer than 8
 * bytes and equal in their first 8 to another such record), out[3] = scratch bytes the call asked for
 * (all 0 when it did not reach its end). */
void tkv_debug_memtable_last(uint64_t out[4]);
/* Which radix passes the calling thread's last tkv_memtable_build_device launched, over all its rounds
 * (pass 0 = the 4 digit bits, 1-8 = the word's bytes from the lowest, 9-12 = the segment's bytes from the
 * lowest): out[0] = OR of 1 << p for every pass one workgroup ran (a list of at most
 * tkv_debug_memtable_geom's out[0] entries), out[1] = the same for passes run as histogram, scan and
 * scatter, out[2] = passes run in the whole build, out[3] = the most levels a histogram scan had (0 when
 * there was none). Cleared when a build starts and recorded on the host as the passes are launched. */
void tkv_debug_memtable_passes(uint64_t out[4]);
/* Phase times of the calling thread's last tkv_memtable_build_device that returned TKV_OK, in
 * milliseconds between device events on its stream: out_ms[0] = the check and the first round, out_ms[1]
 * = the later rounds, out_ms[2] = dedupe (the survivor scans), out_ms[3] = emit (columns, metadata, the
 * arena; with the host's read of the sizes in front). Switch and return value as
 * tkv_debug_sst_build_phases. */
int tkv_debug_memtable_phases(int enable, double out_ms[4]);

/* Outputs one workgroup of tkv_sst_merge_device's merge rounds produces (its tile). Tests place their
 * edges around it. */
uint64_t tkv_debug_sst_merge_tile(void);
/* What the calling thread's last tkv_sst_merge_device did: out[0] = N (input entries), out[1] = merge
 * rounds launched (ceil(log2) of the non-empty runs), out[2] = workgroup tiles of the last round, out[3] =
 * scratch bytes the call asked for (all 0 when it did not reach its end). */
void tkv_debug_sst_merge_last(uint64_t out[4]);
/* Phase times of the calling thread's last tkv_sst_merge_device that returned TKV_OK, in milliseconds
 * between device events on its stream: out_ms[0] = the check pass and the sort entries, out_ms[1] = the
 * merge rounds, out_ms[2] = ties, tombstone drop and the survivor scan, out_ms[3] = emit (with the host's
 * read of the verdict and the sizes in front). Switch and return value as tkv_debug_sst_build_phases. */
int tkv_debug_sst_merge_phases(int enable, double out_ms[4]);

/* Geometry of tkv_sst_get_device: out[0] = queries per workgroup of the search (one lane per query).
 * Tests place their query counts around it. */
void tkv_debug_sst_get_geometry(uint64_t out[1]);
/* What the calling thread's last tkv_sst_get_device did: out[0] = nq, out[1] = n_runs, out[2] = the search
 * steps of the lane that made the most (the sum of ceil(log2(n[r] + 1)) over the runs that lane searched),
 * out[3] = queries FOUND, out[4] = queries DELETED (all 0 when it did not reach its end). */
void tkv_debug_sst_get_last(uint64_t out[5]);
/* Phase times of the calling thread's last tkv_sst_get_device that returned TKV_OK, in milliseconds
 * between device events on its stream: out_ms[0] = the search, out_ms[1] = the two scans, out_ms[2] = the
 * per-query columns and the tile table (with the host's read of the verdicts and the sizes in front),
 * out_ms[3] = the value gather. Switch and return value as tkv_debug_sst_build_phases. */
int tkv_debug_sst_get_phases(int enable, double out_ms[4]);

#ifdef __cplusplus
}
#endif

#endif /* TKV_CRC32_H */
