// What the device DEFLATE encoder (deflate.hip) and the device inflater (inflate.hip) share: the constants of the chunk format that
// include/e2e_hip.h states under N5, and the layout of the inflater's scan records.
#pragma once

namespace e2e {
namespace deflate {

constexpr int CHUNK = 32768;                       // bytes per chunk (<= 65535: a stored block's LEN is 16 bits).  32768 = 127 * 258 + 2:
                                                   // a chunk of one value is 127 matches and a match or two literals
constexpr int STORED_EXTRA = 5;                    // header byte, LEN, NLEN
constexpr int MAX_DISTANCE = 8;                    // the encoder's distances are 1, 2, 4 and 8: a record reads at most 8 bytes in
                                                   // front of itself
enum Kind { STORED = 0, FIXED = 1, DYNAMIC = 2 };  // BTYPE of the chunk's block; what e2e_deflate_encode_dynamic reports in kinds

static_assert(CHUNK % 16 == 0 && CHUNK <= 65535 && CHUNK % MAX_DISTANCE == 0, "one stored block per chunk, whole vectors");

}  // namespace deflate
}  // namespace e2e
