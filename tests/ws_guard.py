"""Guarded scratch workspaces for the workspace-hygiene tests (a plain module: no fixtures, works on CPU tensors too).

vqvae_amd._device.workspace() hands every kernel one grow-only buffer of at least `nbytes + 256` bytes that holds whatever
the previous kernel left in it.  GuardedWorkspace.workspace() is a drop-in that hands out EXACTLY `nbytes`, between two guard
bands, with a payload the test chooses -- so a query that under-reports, an index a little past the last carve and a read of
scratch the call never wrote can all fail a test.  Four modules allocate per call instead (SEAMS: one exact-size torch.empty
behind a module-level `_workspace`); install() replaces those too, so their wrappers get the same guarded, pre-filled bytes.

Payload patterns (all chosen so that no stray read can become an out-of-range address):
  "zeros"   every byte 0
  "ones32"  every 32-bit word 1: an in-range index or count for arrays of >= 2 entries, a set flag, a denormal f32 / f64
  "stale"   (reuse=True) buffers are kept per requested size and handed out again as they are: a call finds what the previous
            call of the same shape left there; a size not seen before starts as "ones32"
"""
import importlib
import sys

import numpy as np
import torch

GUARD = 65536
GUARD_BYTE = 0xC3
FILLS = ("zeros", "ones32", "stale")
# Modules that take their scratch from the caching allocator, one exact-size torch.empty per call, through a module-level
# `_workspace`: (nbytes, dev) everywhere but in cluster, whose `_workspace(dev, n, d, K, S, L)` asks the size query itself.
CLUSTER_SEAM = "vqvae_amd.cluster"
SEAMS = (CLUSTER_SEAM, "vqvae_amd.vae", "vqvae_amd.prior.sampling", "vqvae_amd.baseline.model")


class GuardedWorkspace:
    def __init__(self, fill: str, reuse: bool = False):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
        if (fill == "stale") != bool(reuse):
            raise ValueError('fill "stale" needs reuse=True, and only it reuses buffers')
        self.fill, self.reuse = fill, bool(reuse)
        self.records = []                 # (whole buffer incl. guards, requested size), one per buffer handed out
        self._by_size = {}                # reuse: (device, nbytes) -> whole buffer

    def _new_buffer(self, nbytes: int, dev) -> torch.Tensor:
        # over-allocate by 256 so that the payload can be placed on a 256-byte boundary whatever the allocator returns
        raw = torch.empty(GUARD + nbytes + GUARD + 256, dtype=torch.uint8, device=dev)
        off = (-(raw.data_ptr() + GUARD)) % 256
        buf = raw[off: off + GUARD + nbytes + GUARD]
        buf[:GUARD] = GUARD_BYTE
        buf[GUARD + nbytes:] = GUARD_BYTE
        payload = buf[GUARD: GUARD + nbytes]
        if self.fill == "zeros":
            payload.zero_()
        else:                             # "ones32", and the first sight of a size under "stale"
            payload.zero_()
            payload[0::4] = 1             # little endian: byte 0 of every 32-bit word
        return buf

    def workspace(self, nbytes: int, dev) -> torch.Tensor:
        """Drop-in for vqvae_amd._device.workspace: a uint8 tensor of exactly `nbytes` bytes, 256-byte aligned."""
        nbytes = int(nbytes)
        dev = torch.device(dev)
        key = (dev.type, dev.index, nbytes)
        buf = self._by_size.get(key) if self.reuse else None
        if buf is None:
            buf = self._new_buffer(nbytes, dev)
            self.records.append((buf, nbytes))
            if self.reuse:
                self._by_size[key] = buf
        view = buf[GUARD: GUARD + nbytes]
        assert view.numel() == nbytes
        assert view.data_ptr() % 256 == 0, view.data_ptr()
        return view

    def check(self) -> None:
        """Both guards of every buffer handed out still hold GUARD_BYTE."""
        for buf, nbytes in self.records:
            if buf.is_cuda:
                torch.cuda.synchronize(buf.device)
            for name, lo, band in (("front", -GUARD, buf[:GUARD]), ("back", nbytes, buf[GUARD + nbytes:])):
                bad = torch.nonzero(band != GUARD_BYTE)
                if bad.numel():
                    first = int(bad[0])
                    raise AssertionError(
                        f"workspace of {nbytes} bytes: {name} guard damaged, first at payload offset {lo + first} "
                        f"({int(bad.numel())} bytes changed, byte there 0x{int(band[first]):02x})")

    def _cluster_workspace(self, dev, n, d, K, S=1, L=1) -> torch.Tensor:
        """Drop-in for vqvae_amd.cluster._workspace, which sizes its scratch itself: the same query, the same refusal."""
        from vqvae_amd import _lib
        nbytes = _lib.load().geo_kmeans_workspace_bytes(n, d, K, S, L)
        if nbytes == 0:
            raise _lib.GeoHipError(f"geo_kmeans_workspace_bytes rejected n={n} d={d} K={K} starts={S} trials={L}")
        return self.workspace(nbytes, dev)

    def install(self, monkeypatch) -> set:
        """Replace `workspace` in vqvae_amd._device and in every loaded vqvae_amd.* module that imported it by name, and the
        `_workspace` of the SEAMS modules, which allocate their scratch per call.  Returns the names of the patched modules."""
        for name in ("vqvae_amd.geo", "vqvae_amd._export", "vqvae_amd.geo.analysis") + SEAMS:
            importlib.import_module(name)
        from vqvae_amd import _device
        original = _device.workspace
        if getattr(original, "__self__", None).__class__ is GuardedWorkspace:
            raise RuntimeError("a GuardedWorkspace is already installed")
        patched = set()
        for name, mod in list(sys.modules.items()):
            if mod is None or not (name == "vqvae_amd" or name.startswith("vqvae_amd.")):
                continue
            if getattr(mod, "__dict__", {}).get("workspace") is original:
                monkeypatch.setattr(mod, "workspace", self.workspace)
                patched.add(name)
        assert "vqvae_amd._device" in patched
        for name in SEAMS:
            mod = sys.modules[name]
            seam = vars(mod)["_workspace"]            # a KeyError here: the module lost its seam
            assert callable(seam), (name, seam)
            monkeypatch.setattr(mod, "_workspace", self._cluster_workspace if name == CLUSTER_SEAM else self.workspace)
            patched.add(name)
        return patched


RUNS = (("zeros", False), ("ones32", False), ("stale", True))


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    a = np.ascontiguousarray(x)
    return a.dtype, a.shape, a.tobytes()


def four_runs(monkeypatch, call, A, B, route, compare=None):
    """Run `call` on input B with the allocator in place (P), then guarded on zeros (Z), on ones (O) and -- right after one
    call on input A, which has B's shapes and other data -- on what that call left behind (S).  call(inp) -> (outputs: name ->
    array / number, route).  Asserts intact guards after Z, O and S, `route` in all four runs, and every output of Z, O and S
    equal to P's bit for bit; `compare(name, got, want)` may take over an output by returning True.  Returns P's outputs."""
    want, got_route = call(B)
    assert got_route == route, f"production run: route {got_route}, expected {route}"
    for fill, reuse in RUNS:
        g = GuardedWorkspace(fill, reuse=reuse)
        with monkeypatch.context() as m:
            assert g.install(m)
            if reuse:
                call(A)
                n_first = len(g.records)
            got, got_route = call(B)
            if reuse:            # same shapes, same requests: the call on B found the buffers the call on A left
                assert len(g.records) == n_first, f"input A and B ask for different workspaces ({n_first} -> {len(g.records)})"
        assert g.records, f"{fill}: the wrapper took no workspace from the guarded allocator"
        g.check()
        assert got_route == route, f"{fill}: route {got_route}, expected {route}"
        assert set(got) == set(want)
        for name in want:
            if compare is not None and compare(name, got[name], want[name]):
                continue
            assert _bits(got[name]) == _bits(want[name]), f"{fill}: output '{name}' differs from the production run"
    return want
