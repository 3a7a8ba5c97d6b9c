"""The host half of the chunk walk (backend.chunk_table) against its closed form, the refusal snapshot_chunks keeps, and
the plan calm_cast_bf16 is given — without a GPU."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import calm_vit_dte_amd as calm  # noqa: E402,F401

backend = import_module("calm_vit_dte_amd.backend")
binding = import_module("calm_vit_dte_amd._lib")

CHUNK = 16384


def lengths_cases(c):
    single = [1, c - 1, c, c + 1, 3 * c + 5]
    return [[n] for n in single] + [single, single[::-1], [c + 1, 1, 3 * c + 5, c, c, c - 1, 1]]


@pytest.mark.parametrize("chunk", [CHUNK, 4 * CHUNK, 7])
def test_chunk_table_is_the_cumsum_of_ceil(chunk):
    for lengths in lengths_cases(chunk):
        chunk0, chunk_entry = backend.chunk_table(lengths, chunk)
        per_entry = np.array([-(-n // chunk) for n in lengths])              # ceil(len / chunk)
        ends = np.cumsum(per_entry)
        assert chunk0 == list(ends - per_entry)                               # chunks in front of every entry
        assert len(chunk_entry) == ends[-1]
        # chunk k belongs to the entry whose [chunk0, chunk0 + ceil) holds k: the number of entries that end at or before k
        assert chunk_entry == [int(np.searchsorted(ends, k, side="right")) for k in range(ends[-1])]


def test_the_library_walks_chunks_of_the_size_the_tables_are_built_for():
    lib = binding.load()
    assert int(lib.calm_cast_chunk_elems()) == int(lib.calm_optim_chunk_elems()) == int(lib.calm_ema_chunk_elems()) == CHUNK
    assert int(lib.calm_snapshot_chunk_bytes()) == 4 * CHUNK


@pytest.mark.parametrize("bad", [0, -4])
def test_snapshot_chunks_refuses_an_entry_without_words(bad):
    assert backend.snapshot_chunks([8, 4 * CHUNK + 4], 4 * CHUNK) == backend.chunk_table([8, 4 * CHUNK + 4], 4 * CHUNK)
    with pytest.raises(ValueError, match="snapshot chunk table: entries have at least one word"):
        backend.snapshot_chunks([8, bad, 16], 4 * CHUNK)
    assert backend.chunk_table([8, 0, 16], CHUNK) == ([0, 1, 1], [0, 2])    # an empty optimizer tensor has no chunk


def test_cast_plan_is_a_plan_of_its_own(monkeypatch):
    # (host tensors stand in for device memory: the plan only records addresses)
    monkeypatch.setattr(backend, "_ptr", lambda t, *a, **k: t.data_ptr())
    be = backend.HipBackend()
    chunk = int(be.lib.calm_cast_chunk_elems())
    sizes = [chunk + 1, 7, 3 * chunk + 5]
    pairs = [(torch.zeros(n), torch.zeros(n, dtype=torch.bfloat16)) for n in sizes]
    plan = be.cast_plan(pairs)
    assert isinstance(plan, backend.CastPlan) and not isinstance(plan, backend.SnPlan)
    assert not issubclass(backend.CastPlan, backend.SnPlan) and not issubclass(backend.SnPlan, backend.ChunkPlan)
    assert not hasattr(plan, "blob_dev") and not hasattr(plan, "scratch") and not hasattr(plan, "key")
    ent = plan.table_dev.numpy().view(np.dtype(binding.CastEntry))
    assert plan.n == len(ent) == 3 and plan.n_chunks == 2 + 1 + 4
    assert list(ent["numel"]) == sizes and list(ent["chunk0"]) == [0, 2, 3]
    assert list(ent["src"]) == [s.data_ptr() for s, _ in pairs] and list(ent["dst"]) == [d.data_ptr() for _, d in pairs]
    assert plan.chunk_dev.dtype == torch.int32 and plan.chunk_dev.tolist() == [0, 0, 1, 2, 2, 2, 2]
    with pytest.raises(TypeError, match="cast_plan: contiguous fp32 source / bf16 destination of equal size expected"):
        be.cast_plan([(torch.zeros(8), torch.zeros(9, dtype=torch.bfloat16))])
