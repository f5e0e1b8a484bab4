// Host interface of the device codec for point vectors (point_codec.hip): the zcash/bls12_381
// compressed encodings (48 B G1, 96 B G2) and, below, the uncompressed ones (96 B, 192 B) to and from
// the packed device form a bh_srs holds.  Records are addressed as base + i * stride + offset (bytes,
// multiples of 4), so the interleaved ParameterPair lists of a ceremony contribution are coded in place.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

namespace bh {

void point_codec_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

constexpr size_t compressed_bytes(int group) { return group == BH_G1 ? 48 : 96; }

// n compressed records of `group` at d_raw + i * stride + offset (device memory) -> out (an empty
// bh_srs) in the device form, word for word what srs_from_bytes builds from the same points'
// uncompressed bytes.  Flags, range and squareness are always checked (BH_ERR_INVALID_ENCODING);
// checked adds api.hip's subgroup test (BH_ERR_NOT_IN_SUBGROUP, reported only when no record is
// invalid).  A valid infinity encoding is listed in out->identity_idx, or refused as invalid when
// reject_identity.  Runs on ctx->stream and returns synchronised; the caller holds ctx->mu and has
// set the device.
bh_status points_decompress_device(bh_ctx* ctx, int group, const uint8_t* d_raw, size_t stride, size_t offset,
                                   size_t n, int checked, bool reject_identity, bh_srs* out);
// the same for n consecutive records in host memory
bh_status srs_from_compressed(bh_ctx* ctx, int group, const uint8_t* bytes, size_t n, int checked,
                              bool reject_identity, bh_srs* out);

// points first .. first + n of s -> compressed records at d_out + i * stride + offset (device
// memory); enqueued on ctx->stream, not synchronised.  An identity entry comes out as a non-identity
// record: once the bytes are on the host, points_compress_patch (same arguments, the host copy)
// writes the infinity encoding over each of them.
bh_status points_compress_device(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* d_out, size_t stride,
                                 size_t offset);
void points_compress_patch(const bh_srs* s, size_t first, size_t n, uint8_t* h_out, size_t stride, size_t offset);
// both, into n consecutive records of host memory (synchronised)
bh_status srs_to_compressed(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* out);

// ---- the uncompressed encodings (96 B G1, 192 B G2: the size of the device record), same addressing
constexpr size_t uncompressed_bytes(int group) { return 2 * compressed_bytes(group); }

// BH_POINT_CODEC_HOST=1 in the environment (read at each call) keeps the host loops for the
// uncompressed vector paths, an A/B and diagnostic mode; results do not depend on it.
// point_codec_note records which path the calling thread's last uncompressed vector upload or read
// took (bh_srs_last_codec_device).
bool point_codec_host();
void point_codec_note(bool device);

// n uncompressed records at d_raw + i * stride + offset -> out in the device form, word for word what
// the host parser of srs_from_bytes and k_points_to_dev build.  d_raw may be out->pts itself (stride
// = the record, offset 0): the vector is decoded in place.  Flags and range are always checked;
// checked adds the curve equation and the subgroup test.  Precedence over the whole vector: an
// invalid record (or an identity where reject_identity) BH_ERR_INVALID_ENCODING, else a point off the
// curve BH_ERR_NOT_ON_CURVE, else BH_ERR_NOT_IN_SUBGROUP.  Returns synchronised; the caller holds
// ctx->mu and has set the device.
bh_status points_from_wire_device(bh_ctx* ctx, int group, const uint8_t* d_raw, size_t stride, size_t offset, size_t n,
                                  int checked, bool reject_identity, bh_srs* out);
// the same for n consecutive records in host memory: copied into out->pts and decoded there
bh_status srs_from_wire(bh_ctx* ctx, int group, const uint8_t* bytes, size_t n, int checked, bool reject_identity,
                        bh_srs* out);
// points first .. first + n of s -> uncompressed records (device memory), enqueued on ctx->stream;
// points_wire_patch writes 40 00 ... over the identities in the host copy; srs_to_wire does both
// into n consecutive records of host memory (synchronised)
bh_status points_to_wire_device(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* d_out, size_t stride,
                                size_t offset);
void points_wire_patch(const bh_srs* s, size_t first, size_t n, uint8_t* h_out, size_t stride, size_t offset);
bh_status srs_to_wire(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* out);

}  // namespace bh
