// Training snapshots: gather every state tensor of a run into ONE contiguous buffer (pack) and scatter it back in place
// (unpack), one launch each — the device half of trainer.TrainState.  A torch.save of the same state is one blocking
// device-to-host copy per tensor (~2 700 for Base-224 with the fused optimizer and a weight EMA); here the training
// stream pays one launch and a side stream moves the one buffer.
//   pack    per chunk: packed[offset + b] = tensor[b]
//   unpack  per chunk: tensor[b] = packed[offset + b]
// Work item = chunk of CHUNK_BYTES consecutive bytes of one entry (the walk of chunk_table.h, counted in words).  Bits
// move through integer registers, no arithmetic: NaN payloads and the int32 counters survive.  The packed side of a chunk
// is always 16-byte aligned (offsets and CHUNK_BYTES are multiples of 16, the buffer's base is checked); a chunk whose
// tensor side is 16-byte aligned as well moves 16-byte vectors, U in flight per thread, with a scalar tail; any other
// 4-byte aligned tensor moves single words.  Every word belongs to one thread of one workgroup: no atomics, no workspace;
// the bytes between two entries of the packed buffer are neither written by pack nor read by unpack.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK_WORDS = CHUNK_ELEMS;     // per work item (64 words per thread)
constexpr int CHUNK_BYTES = 4 * CHUNK_WORDS;
constexpr int U = 4;                         // 16-byte vectors a thread has in flight
static_assert(CHUNK_BYTES % 16 == 0, "a chunk starts on a 16-byte boundary of the packed buffer");

// PACK: src = tensor, dst = packed; otherwise the other way round.  The loads of U vectors are issued ahead of the first
// store (src and dst come out of a table: the compiler cannot know that they do not alias).
template <bool PACK>
__global__ __launch_bounds__(NT) void snapshot_move(const calm_snapshot_entry* __restrict__ E,
                                                    const int* __restrict__ chunk_entry, char* packed, long packed_bytes) {
    const calm_snapshot_entry e = E[chunk_entry[blockIdx.x]];
    // a record the host would have refused moves nothing (the table is checked where it is built; this keeps a bad one
    // inside the buffer)
    if (e.offset < 0 || e.nbytes <= 0 || e.offset > packed_bytes || e.nbytes > packed_bytes - e.offset) return;
    const auto [w0, w1] = chunk_span((int)blockIdx.x, CHUNK_WORDS, e.chunk0, e.nbytes >> 2);
    if (w0 < 0) return;
    gu32* t = (gu32*)e.tensor;
    gu32* p = (gu32*)(packed + e.offset);
    const gu32* src = PACK ? t : p;
    gu32* dst = PACK ? p : t;
    if (dev_aligned16(t + w0)) {
        const long v1 = w0 + ((w1 - w0) & ~3L);
        loads_ahead_of_stores<U, 4, NT>(
            w0, v1, [&](long i) __attribute__((always_inline)) { return *(const gu32x4*)(src + i); },
            [&](long i, const u32x4& x) __attribute__((always_inline)) { *(gu32x4*)(dst + i) = x; });
        for (long i = v1 + threadIdx.x; i < w1; i += NT) dst[i] = src[i];
    } else {
        loads_ahead_of_stores<U, 1, NT>(
            w0, w1, [&](long i) __attribute__((always_inline)) { return src[i]; },
            [&](long i, uint32_t x) __attribute__((always_inline)) { dst[i] = x; });
    }
}

template <bool PACK>
int snapshot_launch(const calm_snapshot_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                    int32_t n_chunks, const void* packed, int64_t packed_bytes, void* stream) {
    if (!entries_dev || !chunk_entry_dev || !packed || n_entries <= 0 || n_chunks <= 0 || packed_bytes <= 0)
        return CALM_E_INVAL;
    if ((uintptr_t)packed & 15u) return CALM_E_LAYOUT;
    return calm_launch(snapshot_move<PACK>, n_chunks, NT, 0, stream, entries_dev, chunk_entry_dev, (char*)packed,
                       (long)packed_bytes);
}

}  // namespace

extern "C" {

int32_t calm_snapshot_chunk_bytes(void) { return CHUNK_BYTES; }

int calm_snapshot_pack(const calm_snapshot_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                       int32_t n_chunks, void* packed, int64_t packed_bytes, void* stream) {
    return snapshot_launch<true>(entries_dev, n_entries, chunk_entry_dev, n_chunks, packed, packed_bytes, stream);
}

int calm_snapshot_unpack(const calm_snapshot_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                         int32_t n_chunks, const void* packed, int64_t packed_bytes, void* stream) {
    return snapshot_launch<false>(entries_dev, n_entries, chunk_entry_dev, n_chunks, packed, packed_bytes, stream);
}

}  // extern "C"
