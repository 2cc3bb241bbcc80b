"""tests/ws_guard.py itself, on CPU tensors: the guarded workspace is exact, aligned, notices a byte written outside it, and
its install() reaches every vqvae_amd module that holds `workspace` (a wrapper nobody patched would make
tests/test_gpu_workspace_hygiene.py vacuous); and the four-run harness fails on stand-in wrappers that read scratch they never
wrote or write past the size they asked for."""
import numpy as np
import pytest
import torch

import ws_guard
from ws_guard import GUARD, GUARD_BYTE, GuardedWorkspace

CPU = torch.device("cpu")


def _whole(g, i=-1):
    return g.records[i][0]


@pytest.mark.parametrize("fill", ["zeros", "ones32"])
@pytest.mark.parametrize("nbytes", [4, 256, 1000, 65536 + 12])
def test_view_is_exact_aligned_and_filled(fill, nbytes):
    g = GuardedWorkspace(fill)
    ws = g.workspace(nbytes, CPU)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.is_contiguous()
    assert ws.data_ptr() % 256 == 0
    whole = _whole(g)
    assert whole.numel() == GUARD + nbytes + GUARD and g.records[-1][1] == nbytes
    assert ws.data_ptr() == whole.data_ptr() + GUARD
    assert bool((whole[:GUARD] == GUARD_BYTE).all()) and bool((whole[GUARD + nbytes:] == GUARD_BYTE).all())
    words = ws[: nbytes // 4 * 4].numpy().view(np.int32)
    assert (words == (0 if fill == "zeros" else 1)).all()
    if fill == "ones32":
        assert 0 < float(ws[: nbytes // 4 * 4].numpy().view(np.float32)[0]) < np.finfo(np.float32).tiny      # a denormal
    g.check()
    # every call hands out a fresh buffer, and every one is recorded
    ws2 = g.workspace(nbytes, CPU)
    assert ws2.data_ptr() != ws.data_ptr() and len(g.records) == 2


def test_write_inside_passes_and_one_byte_outside_fails():
    nbytes = 1000
    g = GuardedWorkspace("zeros")
    ws = g.workspace(nbytes, CPU)
    ws.fill_(0x5A)                                          # every byte of the payload, first and last included
    g.check()
    whole = _whole(g)
    whole[GUARD + nbytes] = 0                               # one byte after the payload
    with pytest.raises(AssertionError, match=r"workspace of 1000 bytes: back guard damaged, first at payload offset 1000 "):
        g.check()
    whole[GUARD + nbytes] = GUARD_BYTE
    g.check()
    whole[GUARD - 1] = 0                                    # one byte before it
    with pytest.raises(AssertionError, match=r"workspace of 1000 bytes: front guard damaged, first at payload offset -1 "):
        g.check()
    whole[GUARD - 1] = GUARD_BYTE
    # the damage of an earlier buffer is found after later ones were handed out
    g.workspace(64, CPU)
    whole[0] = 1
    with pytest.raises(AssertionError, match=r"workspace of 1000 bytes: front guard damaged, first at payload offset -65536 "):
        g.check()


def test_stale_hands_the_same_storage_back_unrefilled():
    g = GuardedWorkspace("stale", reuse=True)
    a = g.workspace(512, CPU)
    assert (a.numpy().view(np.int32) == 1).all()            # a size not seen before: ones32
    a.copy_(torch.arange(512, dtype=torch.int64).to(torch.uint8))
    b = g.workspace(512, CPU)
    assert b.data_ptr() == a.data_ptr() and len(g.records) == 1
    assert bool((b == torch.arange(512, dtype=torch.int64).to(torch.uint8)).all())
    c = g.workspace(516, CPU)                               # another size: its own buffer
    assert c.data_ptr() != a.data_ptr() and len(g.records) == 2 and (c.numpy().view(np.int32) == 1).all()
    g.check()


def test_fill_and_reuse_must_agree():
    with pytest.raises(ValueError):
        GuardedWorkspace("stale")
    with pytest.raises(ValueError):
        GuardedWorkspace("zeros", reuse=True)
    with pytest.raises(ValueError):
        GuardedWorkspace("nan")


def test_install_reaches_every_module_that_holds_workspace(monkeypatch):
    import sys
    from vqvae_amd import _device
    original = _device.workspace
    g = GuardedWorkspace("zeros")
    patched = g.install(monkeypatch)
    assert patched
    for name in ("_device", "geo.geo_shortest_paths", "geo.kmeans_optimized", "geo.knn_graph_optimized", "geo.riemannian_metric",
                 "geo.analysis"):
        assert "vqvae_amd." + name in patched, (name, sorted(patched))
    # no loaded module of the package still holds the original
    holders = {name: mod for name, mod in sys.modules.items()
               if mod is not None and (name == "vqvae_amd" or name.startswith("vqvae_amd.")) and "workspace" in vars(mod)}
    assert set(holders) == patched, (sorted(holders), sorted(patched))
    for name, mod in holders.items():
        assert mod.workspace is not original and mod.workspace.__self__ is g, name
    # capped_workspace looks `workspace` up at call time: the _device patch must reach it
    from vqvae_amd import _export
    ws = _export.capped_workspace(1000, None, CPU, "test")
    assert ws.numel() == 1000 and len(g.records) == 1 and ws.data_ptr() == g.records[0][0].data_ptr() + GUARD
    with pytest.raises(RuntimeError):
        GuardedWorkspace("ones32").install(monkeypatch)     # one at a time
    monkeypatch.undo()
    assert all(mod.workspace is original for mod in holders.values())
    assert ws_guard.FILLS == ("zeros", "ones32", "stale")


# ---- the four-run harness, on stand-in "kernels" that misuse their scratch in the ways it exists to catch ---------------------
def _fake_wrapper(kind):
    """A wrapper in the style of vqvae_amd.geo: n float32 partial sums and one int32 counter in scratch from _device.workspace."""
    def call(x):
        from vqvae_amd import _device
        n = x.numel()
        query = 4 * n + (0 if kind == "query_under_reports" else 4)
        ws = _device.workspace(query, CPU)
        whole = torch.as_strided(ws, (4 * n + 4,), (1,))        # what the "kernel" addresses, whatever the query answered
        acc, cnt = whole[: 4 * n].view(torch.float32), whole[4 * n:].view(torch.int32)
        if kind != "reads_unwritten_sums":
            acc.zero_()
        if kind != "reads_unwritten_counter":
            cnt.zero_()
        acc += x
        cnt += 1
        return {"sum": acc.clone(), "count": cnt.clone()}, kind
    return call


def _harness(monkeypatch, kind):
    from vqvae_amd import _device
    # the production allocator needs a GPU stream: stand in for it with what it hands out in a fresh process -- zeros, 256 spare
    monkeypatch.setattr(_device, "workspace", lambda nbytes, dev: torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=dev))
    A, B = torch.arange(1.0, 9.0), torch.arange(9.0, 17.0)
    return ws_guard.four_runs(monkeypatch, _fake_wrapper(kind), A, B, kind)


def test_four_runs_pass_a_wrapper_that_writes_what_it_reads(monkeypatch):
    out = _harness(monkeypatch, "clean")
    assert torch.equal(out["sum"], torch.arange(9.0, 17.0)) and int(out["count"]) == 1


def test_four_runs_catch_an_unwritten_counter_on_ones(monkeypatch):
    with pytest.raises(AssertionError, match="ones32: output 'count' differs"):
        _harness(monkeypatch, "reads_unwritten_counter")


def test_four_runs_catch_unwritten_floats_on_stale_scratch_only(monkeypatch):
    """A float32 denormal vanishes in a sum: zeros and ones pass, the leftovers of input A do not."""
    with pytest.raises(AssertionError, match="stale: output 'sum' differs"):
        _harness(monkeypatch, "reads_unwritten_sums")


def test_four_runs_catch_a_query_that_leans_on_the_spare_bytes(monkeypatch):
    with pytest.raises(AssertionError, match="workspace of 32 bytes: back guard damaged, first at payload offset 32 "):
        _harness(monkeypatch, "query_under_reports")


def test_four_runs_assert_the_route(monkeypatch):
    from vqvae_amd import _device
    monkeypatch.setattr(_device, "workspace", lambda nbytes, dev: torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=dev))
    with pytest.raises(AssertionError, match="route clean, expected other"):
        ws_guard.four_runs(monkeypatch, _fake_wrapper("clean"), torch.ones(4), torch.ones(4), "other")
