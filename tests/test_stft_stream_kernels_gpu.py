"""The streaming STFT front-end (csrc/stft_stream.hip and csrc/stream_product.h behind ``ops.stft_stream`` and
``avvad_stft_stream_fwd`` / ``_fwd_spec``) on the MI355X against tests/stft_stream_ref.py: every case of its tiers through the
HIP path, one case under one policy per test id, with nothing here but the HIP implementation of one call -- through
``ops.stft_stream`` and a ``SampleClock`` where the call is one that op builds, through ``avvad._lib`` where the descriptor or
the counts are the test's own, out of one guarded arena for the clamp cases -- and calls into the assertion functions."""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_stream_ref as S
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
PATTERN = 777.25                                          # what the guard bands of the arena hold


class Hip:
    """``impl(call)`` of stft_stream_ref on the GPU"""

    def __init__(self):
        self.bases, self.clock = {}, None

    def basis(self, n_fft):
        from avvad import ops
        if n_fft not in self.bases:
            self.bases[n_fft] = ops.stft_stream_basis(n_fft, DEV)
        return self.bases[n_fft]

    def __call__(self, call):
        cfg = call["cfg"]
        stats = (T_(cfg["mean"]).to(DEV), T_(cfg["std"]).to(DEV)) if call["stats"] else (None, None)
        peak = None if call["peak"] is None else T_(call["peak"]).to(DEV)
        if call["arena"]:
            return self.direct(call, peak, stats, arena=True)
        return self.through_ops(call, peak, stats) if call["plain"] else self.direct(call, peak, stats)

    def through_ops(self, call, peak, stats):
        from avvad import ops
        from avvad.stream import SampleClock
        cfg = call["cfg"]
        B, K = call["state_in"].shape
        if call["first"]:
            self.clock = SampleClock(B, K, cfg["hop"])
        assert self.clock.pending == call["n_pending"], "the SampleClock and the header's bookkeeping disagree"
        state = T_(call["state_in"]).to(DEV)
        spare = torch.full_like(state, float("nan"))
        res = ops.stft_stream(T_(call["chunk"]).to(DEV), call["n_valid"], self.clock, state, self.basis(K), peak, stats[0], stats[1],
                              list(call["final"]), spare, eps=cfg["eps"], norm_eps=cfg["norm_eps"], return_spec=call["spec"])
        assert res[1] == call["n_frames"], "the SampleClock and the header's bookkeeping disagree"
        return dict(out=res[0].cpu().numpy(), spec=res[2].cpu().numpy() if call["spec"] else None, state=spare.cpu().numpy())

    def direct(self, call, peak, stats, arena=False):
        """the C entry point with the call's own descriptor; ``arena``: chunk, both states, out and spec lie in ONE allocation
        with guard bands of 4 n_fft floats between and around them"""
        from avvad import _lib as L
        cfg = call["cfg"]
        B, K = call["state_in"].shape
        Lp, T, F = call["chunk"].shape[1], call["T"], K // 2 + 1
        sizes = dict(chunk=B * Lp, state_in=B * K, state_out=B * K, out=B * T * F, spec=B * T * F * 2)
        G = 4 * K if arena else 0
        offs, at = {}, G
        for k, n in sizes.items():
            offs[k] = at
            at += -(-max(n, 1) // 64) * 64 + G
        mem = torch.full((at,), PATTERN if arena else float("nan"), dtype=torch.float32, device=DEV)
        view = lambda k: mem[offs[k]:offs[k] + sizes[k]]
        view("chunk").copy_(T_(call["chunk"]).reshape(-1))
        view("state_in").copy_(T_(call["state_in"]).reshape(-1))
        for k in ("state_out", "out", "spec"):
            view(k).fill_(float("nan"))
        counts = torch.tensor([call["n_valid"], call["n_pending"], call["n_frames"], call["pad"]], dtype=torch.int32).to(DEV)
        d = L.StftStreamDesc(B, Lp, K, cfg["hop"], T, call["M"], float(cfg["eps"]), float(cfg["norm_eps"]))
        args = [L.ptr(view("chunk")), L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(counts[2]), L.ptr(counts[3]), L.ptr(peak),
                L.ptr(view("state_in")), L.ptr(view("state_out")), L.ptr(self.basis(K)), L.ptr(stats[0]), L.ptr(stats[1]),
                L.ptr(view("out")) if T else None]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if call["spec"]:
            rc = L.lib().avvad_stft_stream_fwd_spec(*args, L.ptr(view("spec")) if T else None, C.byref(d), stream)
        else:
            rc = L.lib().avvad_stft_stream_fwd(*args, C.byref(d), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        host = mem.cpu().numpy()
        get = lambda k, shape: host[offs[k]:offs[k] + sizes[k]].reshape(shape).copy()
        g = dict(out=get("out", (B, T, F)), spec=get("spec", (B, T, F, 2)) if call["spec"] else None, state=get("state_out", (B, K)))
        assert np.array_equal(S.bits(get("chunk", (B, Lp))), S.bits(call["chunk"])), "the chunk was written"
        assert np.array_equal(S.bits(get("state_in", (B, K))), S.bits(call["state_in"])), "state_in was written"
        if arena:
            names = list(sizes)
            lo = [0] + [offs[k] + sizes[k] for k in names]                # a band starts where the buffer in front of it ends
            hi = [offs[k] for k in names] + [at]
            g["guards"] = [("in front of " + names[i] if i < len(names) else "behind " + names[-1],
                            bool((host[lo[i]:hi[i]] == np.float32(PATTERN)).all()) and hi[i] - lo[i] >= G) for i in range(len(lo))]
        return g


HIP = Hip()
CACHE = {}
IMPULSE_COUNT = [0, 0]


@pytest.mark.parametrize("name,policy", S.IMPULSE + S.GRID)
def test_impulse_tier(name, policy):
    off, total = S.check_impulse(HIP, name, policy)
    assert total > 0
    IMPULSE_COUNT[0] += off
    IMPULSE_COUNT[1] += total


@pytest.mark.parametrize("name,policy", S.ROUNDING)
def test_rounding_tier(name, policy):
    fig = S.check_rounding(HIP, name, policy, cache=CACHE)
    assert fig["worst"] > 0


@pytest.mark.parametrize("name,policy", S.FEATURES)
def test_feature_tier(name, policy):
    S.check_features(HIP, name, policy, cache=CACHE)


@pytest.mark.parametrize("name,policy", S.SILENCE)
def test_silence(name, policy):
    S.check_silence(HIP, name, policy)


@pytest.mark.parametrize("n_fft,hop", S.DIRECT)
def test_direct_calls(n_fft, hop):
    S.check_direct(HIP, n_fft, hop)


@pytest.mark.parametrize("variant", S.CLAMP_VARIANTS)
@pytest.mark.parametrize("n_fft,hop", S.DIRECT)
def test_clamped_counts_stay_inside_their_buffers(n_fft, hop, variant):
    r = S.check_clamp(HIP, n_fft, hop, variant)
    assert len(r["counts"]) == 3


def test_zz_log_worst_ratios():
    for (tag, tier), (ratio, name) in sorted(S.FIGS.items()):
        if tag == "gpu":
            S.H.log_line("stft_stream gpu      WORST %-32s %.4f  (%s)" % (tier, ratio, name))
    S.H.log_line("stft_stream gpu      impulse tier: %d of %d non-zero elements off float32(reference)" % tuple(IMPULSE_COUNT))
