"""numpy emulation of calm_snapshot_pack / calm_snapshot_unpack (csrc/snapshot.hip), walking the chunk table the way the
kernels do — chunk k belongs to entry chunk_entry[k] and moves its words [(k - chunk0) * C, min(.. + C, nwords)) — and
the table of tensors the snapshot tests share: every size at which the kernels take another path, as views at word
offsets 0 .. 3 into larger bases (so that the tensor side of a chunk is and is not 16-byte aligned) with guard words in
front and behind, fp32 and int32, NaN payloads and denormals among the bit patterns."""
import numpy as np
import torch

GUARD = 8                      # words in front of and behind every view
SENTINEL = 0xA5                # what padding bytes of a packed buffer hold before a pack
NAN_BITS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff800001, 0x00000001, 0x807fffff, 0x00400000, 0x80000000],
                    dtype=np.uint32)   # quiet / signalling NaNs with payloads, denormals, -0


def sizes_in_words(chunk_words):
    C = chunk_words
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7]


def make_table(chunk_words, device, seed=0, many=0):
    """[(name, tensor)]: for every size and every word offset 0 .. 3 one fp32 or int32 view (dtypes alternate), plus one
    tensor without elements; `many` > 0 adds that many small entries (a table of more than 1 024).  Every tensor is a
    view into a base with GUARD words on either side."""
    rng = np.random.default_rng(seed)
    out = []

    def view(name, n, shift, as_int):
        bits = rng.integers(0, 1 << 32, n + 2 * GUARD + 4, dtype=np.uint64).astype(np.uint32)
        k = min(len(NAN_BITS), n)
        bits[GUARD + shift:GUARD + shift + k] = NAN_BITS[:k]              # first words of the view
        bits[GUARD + shift + n - k:GUARD + shift + n] = NAN_BITS[:k][::-1]  # and its last ones (the tail paths)
        base = torch.from_numpy(bits.view(np.int32).copy()).to(device)
        if not as_int:
            base = base.view(torch.float32)
        t = base[GUARD + shift:GUARD + shift + n]
        assert t._base is base
        out.append((name, t))

    i = 0
    for n in sizes_in_words(chunk_words):
        for shift in range(4):
            view(f"t{n}_s{shift}", n, shift, as_int=i % 2 == 1)
            i += 1
    out.insert(3, ("empty", torch.zeros(0, dtype=torch.float32, device=device)))
    for j in range(many):
        view(f"m{j}", 1 + j % 7, j % 4, as_int=j % 3 == 0)
    return out


def words(t):
    """The bits of a tensor as a numpy uint32 array (host copy)."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32).numpy().view(np.uint32).copy()


def base_words(t):
    return words(t._base)


def live(entries, offsets, sizes):
    """The entries with elements and their (offset, nbytes): what gets a table record."""
    return [(n, t, off, nb) for (n, t), off, nb in zip(entries, offsets, sizes) if nb > 0]


def emulate_pack(arrays, offsets, sizes, chunk0, chunk_entry, chunk_bytes, packed):
    """arrays: uint32 arrays of the live entries; packed: uint8 array, written in place chunk by chunk."""
    CW = chunk_bytes // 4
    p32 = packed.view(np.uint32)
    moved = 0
    for k, e in enumerate(chunk_entry):
        w0 = (k - chunk0[e]) * CW
        w1 = min(w0 + CW, sizes[e] // 4)
        assert 0 <= w0 < w1, "a chunk without words"
        assert offsets[e] % 16 == 0 and offsets[e] + 4 * w1 <= packed.size
        p32[offsets[e] // 4 + w0:offsets[e] // 4 + w1] = arrays[e][w0:w1]
        moved += w1 - w0
    assert moved == sum(s // 4 for s in sizes), "every word belongs to exactly one chunk"
    return packed


def emulate_unpack(arrays, offsets, sizes, chunk0, chunk_entry, chunk_bytes, packed):
    CW = chunk_bytes // 4
    p32 = packed.view(np.uint32)
    for k, e in enumerate(chunk_entry):
        w0 = (k - chunk0[e]) * CW
        w1 = min(w0 + CW, sizes[e] // 4)
        arrays[e][w0:w1] = p32[offsets[e] // 4 + w0:offsets[e] // 4 + w1]
    return arrays


def payload_mask(offsets, sizes, packed_bytes):
    """bool [packed_bytes]: True on the bytes that belong to an entry."""
    m = np.zeros(packed_bytes, dtype=bool)
    for off, nb in zip(offsets, sizes):
        m[off:off + nb] = True
    return m
