"""tests/ws_guard.py itself, on CPU tensors: the guarded workspace is exact, aligned, notices a byte written outside it, and
its install() reaches every vqvae_amd module that holds `workspace` (a wrapper nobody patched would make
tests/test_gpu_workspace_hygiene.py vacuous) and the `_workspace` of the four modules that allocate per call
(ws_guard.SEAMS); and the four-run harness fails on stand-in wrappers, behind either kind of allocator, that read scratch they
never wrote, write past the size they asked for, or take no guarded workspace at all."""
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
    assert set(holders) == patched - set(ws_guard.SEAMS), (sorted(holders), sorted(patched))
    assert not set(holders) & set(ws_guard.SEAMS)
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


# ---- the per-call allocators (ws_guard.SEAMS): cluster, vae, prior.sampling and baseline.model -----------------------------
KM_SHAPE = (129, 17, 33)                                    # cluster._workspace sizes its scratch itself: (n, d, K)


def _seam(name):
    import importlib
    return importlib.import_module(name)


def _kmeans_bytes():
    from vqvae_amd import _lib
    nbytes = _lib.load().geo_kmeans_workspace_bytes(*KM_SHAPE, 1, 1)
    assert nbytes > 4096
    return nbytes


def _take(name, nbytes):
    """Scratch of `nbytes` bytes from the module's seam, asked for as its wrapper asks: cluster's seam takes the problem's shape
    and answers geo_kmeans_workspace_bytes of it, so there `nbytes` must be _kmeans_bytes()."""
    mod = _seam(name)
    if name == ws_guard.CLUSTER_SEAM:
        assert nbytes == _kmeans_bytes()
        return mod._workspace(CPU, *KM_SHAPE)
    return mod._workspace(nbytes, CPU)


@pytest.mark.parametrize("name", ws_guard.SEAMS)
def test_production_seam_is_one_exact_allocation(name):
    nbytes = _kmeans_bytes() if name == ws_guard.CLUSTER_SEAM else 1000
    ws = _take(name, nbytes)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.is_contiguous() and ws.storage_offset() == 0
    assert ws.untyped_storage().nbytes() == nbytes


def test_install_patches_the_four_seams_and_reports_them(monkeypatch):
    originals = {name: _seam(name)._workspace for name in ws_guard.SEAMS}
    g = GuardedWorkspace("ones32")
    patched = g.install(monkeypatch)
    assert set(ws_guard.SEAMS) <= patched and len(ws_guard.SEAMS) == 4
    for i, name in enumerate(ws_guard.SEAMS):
        assert _seam(name)._workspace is not originals[name] and _seam(name)._workspace.__self__ is g, name
        nbytes = _kmeans_bytes() if name == ws_guard.CLUSTER_SEAM else 1000 + 4 * i
        ws = _take(name, nbytes)
        assert ws.numel() == nbytes and ws.data_ptr() % 256 == 0 and len(g.records) == i + 1 and g.records[-1][1] == nbytes
        assert ws.data_ptr() == _whole(g).data_ptr() + GUARD and (ws.numpy().view(np.int32) == 1).all()
    g.check()
    # a size the library refuses is refused under the guard as in production
    from vqvae_amd import _lib
    with pytest.raises(_lib.GeoHipError, match="geo_kmeans_workspace_bytes rejected"):
        _seam(ws_guard.CLUSTER_SEAM)._workspace(CPU, 100, 129, 4)
    monkeypatch.undo()
    assert all(_seam(name)._workspace is originals[name] for name in ws_guard.SEAMS)


def _fake_seam_wrapper(name, kind):
    """_fake_wrapper for a module that allocates per call: n float32 partial sums at the front of its scratch, one int32 counter
    in its last word -- or, when the query under-reports, in the word after it."""
    def call(x):
        n = x.numel()
        if name == ws_guard.CLUSTER_SEAM:
            query = _kmeans_bytes()
            cnt_at = query if kind == "query_under_reports" else query - 4
        else:
            cnt_at = 4 * n
            query = cnt_at + (0 if kind == "query_under_reports" else 4)
        ws = _take(name, query)
        whole = torch.as_strided(ws, (cnt_at + 4,), (1,))          # what the "kernel" addresses, whatever the query answered
        acc, cnt = whole[: 4 * n].view(torch.float32), whole[cnt_at:].view(torch.int32)
        if kind != "reads_unwritten_sums":
            acc.zero_()
        if kind != "reads_unwritten_counter":
            cnt.zero_()
        acc += x
        cnt += 1
        return {"sum": acc.clone(), "count": cnt.clone()}, kind
    return call


def _seam_harness(monkeypatch, name, kind):
    # stand-ins for the caching allocator in a fresh process: zeros, and (as its 512-byte blocks leave) spare bytes behind
    def zeros(nbytes, dev):
        return torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=dev)[:int(nbytes)]
    if name == ws_guard.CLUSTER_SEAM:
        monkeypatch.setattr(_seam(name), "_workspace", lambda dev, n, d, K, S=1, L=1: zeros(_kmeans_bytes(), dev))
    else:
        monkeypatch.setattr(_seam(name), "_workspace", zeros)
    A, B = torch.arange(1.0, 9.0), torch.arange(9.0, 17.0)
    return ws_guard.four_runs(monkeypatch, _fake_seam_wrapper(name, kind), A, B, kind)


@pytest.mark.parametrize("name", ws_guard.SEAMS)
def test_four_runs_reach_a_wrapper_behind_a_seam(name, monkeypatch):
    out = _seam_harness(monkeypatch, name, "clean")
    assert torch.equal(out["sum"], torch.arange(9.0, 17.0)) and int(out["count"]) == 1


@pytest.mark.parametrize("name", ws_guard.SEAMS)
def test_four_runs_catch_an_unwritten_word_behind_a_seam(name, monkeypatch):
    with pytest.raises(AssertionError, match="ones32: output 'count' differs"):
        _seam_harness(monkeypatch, name, "reads_unwritten_counter")
    with pytest.raises(AssertionError, match="stale: output 'sum' differs"):
        _seam_harness(monkeypatch, name, "reads_unwritten_sums")


@pytest.mark.parametrize("name", ws_guard.SEAMS)
def test_four_runs_catch_a_seam_request_that_leans_on_spare_bytes(name, monkeypatch):
    nbytes = _kmeans_bytes() if name == ws_guard.CLUSTER_SEAM else 32
    with pytest.raises(AssertionError, match=rf"workspace of {nbytes} bytes: back guard damaged, first at payload offset {nbytes} "):
        _seam_harness(monkeypatch, name, "query_under_reports")


def test_four_runs_fail_a_wrapper_that_takes_no_guarded_workspace(monkeypatch):
    """A wrapper that went back to an inline torch.empty is not a case that passes: it is a case that fails."""
    def call(x):
        ws = torch.zeros(4 * x.numel(), dtype=torch.uint8)
        return {"sum": ws.view(torch.float32) + x}, "inline"
    with pytest.raises(AssertionError, match="zeros: the wrapper took no workspace from the guarded allocator"):
        ws_guard.four_runs(monkeypatch, call, torch.ones(4), torch.ones(4), "inline")
