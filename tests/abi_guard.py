"""Poisoned, guarded buffers for the caller-owned buffer contract of include/avvad.h.

The C ABI says "the caller allocates every buffer, including the workspace".  Three things follow, and this helper
makes each of them observable:

  (a) what a workspace or an output holds on entry never reaches a result;
  (b) nothing outside ``[ws, ws + ws_bytes)`` is written;
  (c) a workspace below the queried size is refused before anything is launched.

``Guard`` hands out workspaces that are views into a larger tensor with ``GUARD`` floats of the same fill pattern on
either side, and fills every float32 output with that pattern; ``guarded(...)`` installs one in ``avvad.ops`` for the
duration of a ``with`` block (``ops._ws``, ``ops.engine_ws`` and the ``empty`` / ``empty_like`` of the name ``torch`` AS
``ops`` SEES IT -- the real ``torch`` module is not touched).  Cases that call the library directly use the same
``Guard`` through ``workspace()`` / ``output()``.

``run_contract`` is the protocol every case goes through: three runs (zeros, quiet NaN, the finite 1e30), results equal
bit for bit across the fills, guards intact, and a fourth run with a workspace one float short that must be refused
with every registered buffer still poisoned -- one such run per entry point the case goes through.  A backward entry
point gets its short run from ``expect_backward_refused``.

A plain module: no fixtures, no pytest settings.
"""
import contextlib
import ctypes
import math

import torch

GUARD = 65536                  # floats on either side: a whole 128x128 tile, and a multiple of 64 floats (256 bytes)
FILLS = (("zero", 0.0), ("nan", float("nan")), ("big", 1e30))


class GuardError(AssertionError):
    pass


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pattern_bits(fill):
    return int(_bits(torch.full((1,), fill, dtype=torch.float32))[0])


class Guard:
    """Registry of the buffers handed out during one run.  ``fill``: the float every guard, workspace body and output is
    set to.  ``short``: workspaces come back one float shorter than asked for (the rear guard starts right behind them)."""

    def __init__(self, fill, short=False, offset=0):
        self.fill = float(fill)
        self.short = bool(short)
        self.offset = int(offset)  # floats by which a workspace is moved off its 256-byte boundary (alignment cases)
        self.bits = _pattern_bits(self.fill)
        self.workspaces = []       # (owner, start, n): owner = [GUARD + offset | n floats | GUARD]
        self.outputs = []

    # ------------------------------------------------------------------ allocation
    def workspace(self, nfloats, device):
        """A ``nfloats``-float (``nfloats - 1`` when short) view, 256-byte aligned like torch's own blocks."""
        nfloats = int(nfloats)
        n = nfloats - 1 if self.short else nfloats
        if n < 0:
            raise ValueError("workspace of %d floats cannot be shortened" % nfloats)
        start = GUARD + self.offset
        owner = torch.full((start + n + GUARD,), self.fill, dtype=torch.float32, device=device)
        self.workspaces.append((owner, start, n))
        return owner[start:start + n]

    def workspace_bytes(self, nbytes, device):
        return self.workspace((int(nbytes) + 3) // 4, device)

    def output(self, t):
        """Poison and register an output tensor (float32 only; anything else is returned as it is)."""
        if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
            t.fill_(self.fill)
            self.outputs.append(t)
        return t

    def new_output(self, *shape, device):
        return self.output(torch.empty(*shape, dtype=torch.float32, device=device))

    # ------------------------------------------------------------------ checks
    def _bad(self, t):
        """number of floats of ``t`` that do not hold the pattern bit for bit, and the first such index"""
        if t.numel() == 0:
            return 0, -1
        ne = _bits(t).reshape(-1) != self.bits
        n = int(ne.sum())
        return n, (int(ne.nonzero()[0]) if n else -1)

    def check(self):
        """Every guard still holds its pattern bit for bit."""
        for i, (owner, start, n) in enumerate(self.workspaces):
            nb, at = self._bad(owner[:start])
            if nb:
                raise GuardError("workspace %d (%d floats): %d floats written BEFORE it, the nearest %d floats in front"
                                 % (i, n, nb, start - int((_bits(owner[:start]).reshape(-1) != self.bits).nonzero()[-1])))
            nb, at = self._bad(owner[start + n:])
            if nb:
                raise GuardError("workspace %d (%d floats): %d floats written BEHIND it, the first %d floats past its end"
                                 % (i, n, nb, at))

    def assert_untouched(self):
        """Every registered buffer -- guards, workspace bodies, outputs -- still holds its pattern: nothing was launched."""
        for i, (owner, start, n) in enumerate(self.workspaces):
            nb, at = self._bad(owner)
            if nb:
                raise GuardError("workspace %d: %d floats changed (first at %d of the guarded block) although the call was "
                                 "refused" % (i, nb, at))
        for i, t in enumerate(self.outputs):
            nb, at = self._bad(t)
            if nb:
                raise GuardError("output %d %s: %d floats changed although the call was refused" % (i, tuple(t.shape), nb))


class _TorchProxy:
    """Stands in for the name ``torch`` inside ``avvad.ops``: ``empty`` / ``empty_like`` poison and register what they
    return, every other attribute is the real module's (``zeros`` / ``zeros_like`` included: those tensors are state)."""

    def __init__(self, real, guard):
        self.__dict__["_real"] = real
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *a, **k):
        return self._guard.output(self._real.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._guard.output(self._real.empty_like(*a, **k))


@contextlib.contextmanager
def guarded(monkeypatch, ops, fill, short=False, engine_floats=None, offset=0):
    """Install a ``Guard`` in the module ``ops`` until the block ends; yields it.  ``engine_floats``: size of
    ``ops.engine_ws`` (default: the library's ``avvad_engine_workspace()``, asked when first needed)."""
    g = Guard(fill, short, offset)

    def _ws(nbytes, device):
        if nbytes == 0:
            raise ops.L.AvvadError("workspace query failed (bad descriptor)")
        return g.workspace_bytes(nbytes, device)

    def engine_ws(device):
        n = engine_floats if engine_floats is not None else ops.L.lib().avvad_engine_workspace() // 4
        return g.workspace(n, device)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "_ws", _ws)
        mp.setattr(ops, "engine_ws", engine_ws)
        mp.setattr(ops, "torch", _TorchProxy(torch, g))
        yield g


def _same(name, a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s: shape / dtype differ (%s %s vs %s %s)" % (name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    if torch.equal(a, b):
        return None
    d = (a.double() - b.double())
    n = int((_bits(a) != _bits(b)).sum()) if a.dtype == torch.float32 else int((a != b).sum())
    return "%s: %d of %d values differ, max|d| = %s" % (name, n, a.numel(), float(d.abs().nan_to_num(nan=math.inf).max()))


def run_contract(monkeypatch, ops, case, short="refused", short_ops=None, error=None, match="AVVAD_EWORKSPACE", engine_floats=None):
    """The protocol of one case.  ``case()`` runs the operation on inputs built once (outside) and returns a dict
    name -> result tensor (outputs and gradients), leaving no state behind that a second call would see.

    Runs it under the three fills, asserts the guards after each, asserts the NaN and 1e30 results equal the zero run
    (``torch.equal``), then -- unless ``short`` is None -- with workspaces one float short: ``"refused"`` expects ``error``
    (default ``ops.L.AvvadError``) matching ``match`` and every registered buffer untouched.  A refused call raises, so a
    case that goes through several entry points names each of them in ``short_ops``, a dict name -> callable that
    reaches that entry point FIRST; every one gets a short run of its own (default: the case itself, for one entry
    point).  Returns the NaN run's results, for the comparison with the op's reference."""
    res = {}
    for tag, fill in FILLS:
        with guarded(monkeypatch, ops, fill, engine_floats=engine_floats) as g:
            out = case()
            out = {k: v.detach().clone() for k, v in out.items()}
            g.check()
        if not g.workspaces and not g.outputs:
            raise GuardError("the case allocated nothing through ops: the harness saw no buffer")
        res[tag] = out
    for tag in ("nan", "big"):
        if res[tag].keys() != res["zero"].keys():
            raise GuardError("result names differ between fills")
        for k in res["zero"]:
            msg = _same(k, res[tag][k], res["zero"][k])
            if msg:
                raise GuardError("fill %r changes a result (buffer contents on entry reached it) -- %s" % (tag, msg))
    if short == "refused":
        for name, op in (short_ops or {"case": case}).items():
            try:
                expect_refused(monkeypatch, ops, op, match, short=True, error=error, engine_floats=engine_floats)
            except GuardError as e:
                raise GuardError("%s: %s" % (name, e))
    elif short is not None:
        raise ValueError(short)
    return res["nan"]


def expect_refused(monkeypatch, ops, case, match, short=False, offset=0, error=None, engine_floats=None):
    """``case()`` with workspaces one float short (``short``) or ``offset`` floats off their alignment must raise ``error``
    (default ``ops.L.AvvadError``) whose text holds ``match``, with every registered buffer still poisoned (NaN)."""
    what = "short workspace" if short else "workspace %d bytes off its alignment" % (4 * offset)
    err = error if error is not None else ops.L.AvvadError
    with guarded(monkeypatch, ops, FILLS[1][1], short=short, engine_floats=engine_floats, offset=offset) as g:
        try:
            case()
        except err as e:
            if match not in str(e):
                raise GuardError("%s: refused, but not as %s: %s" % (what, match, e))
        else:
            raise GuardError("%s: the call was NOT refused (no %s)" % (what, match))
        if not g.workspaces:
            raise GuardError("%s: the case asked for no workspace" % what)
        g.assert_untouched()


def expect_backward_refused(monkeypatch, ops, entry, forward, backward, match="AVVAD_EWORKSPACE", misaligned=False):
    """The backward entry point ``entry`` (a name in the library) with the forward's workspace declared one float short
    (``misaligned``: with the workspace pointer, the argument before ``ws_bytes``, 4 bytes further on instead).
    ``ops`` hands a backward the tensor its forward kept, so the size cannot be shortened through the allocator: the
    library call itself is wrapped, and its ``ws_bytes`` (the argument before the stream, on every entry point) goes in 4
    bytes lower.  ``forward()`` runs under a NaN guard and returns what ``backward(...)`` needs; that must raise
    ``ops.L.AvvadError`` holding ``match``, and across the library call no registered buffer may change by a bit: the
    workspace the forward filled, its guards, the forward's outputs and the gradient buffers allocated for this call."""
    with guarded(monkeypatch, ops, FILLS[1][1]) as g:
        kept = forward()
        lib = ops.L.lib()
        real = getattr(lib, entry)
        calls = []

        def one_float_short(*a):
            if calls:                             # (a stack of layers: the first call was refused, nothing follows it)
                raise GuardError("%s was called again after it had refused" % entry)
            held = [(t, _bits(t).clone()) for t in [o for o, _, _ in g.workspaces] + g.outputs]
            if misaligned:
                rc = real(*(a[:-3] + (ctypes.c_void_p(a[-3].value + 4),) + a[-2:]))
            else:
                rc = real(*(a[:-2] + (a[-2] - 4,) + a[-1:]))
            calls.append(rc)
            for t, bits in held:
                if rc and not torch.equal(_bits(t), bits):
                    raise GuardError("%s refused (%d), but a buffer of %d floats changed: it launched "
                                     "before it refused" % (entry, rc, t.numel()))
            return rc
        with monkeypatch.context() as mp:
            mp.setattr(lib, entry, one_float_short)
            try:
                backward(kept)
            except ops.L.AvvadError as e:
                if match not in str(e):
                    raise GuardError("%s: refused, but not as %s: %s" % (entry, match, e))
            else:
                raise GuardError("%s: the call was NOT refused (no %s)" % (entry, match))
        if not calls:
            raise GuardError("%s was never reached" % entry)
        g.check()


def run_direct(case):
    """The direct-ABI twin of ``run_contract`` for cases that call the library themselves: ``case(g)`` takes its
    workspaces from ``g.workspace`` / ``g.workspace_bytes`` and its outputs from ``g.new_output`` and returns the dict of
    results.  Three fills, guards intact, results equal across the fills; returns the NaN run's results.  What a short
    workspace must do is the case's own business (the engine's documented whole-tile fallback, for one)."""
    res = {}
    for tag, fill in FILLS:
        g = Guard(fill)
        out = {k: v.detach().clone() for k, v in case(g).items()}
        g.check()
        if not g.workspaces and not g.outputs:
            raise GuardError("the case took no buffer from the guard")
        res[tag] = out
    for tag in ("nan", "big"):
        for k in res["zero"]:
            msg = _same(k, res[tag][k], res["zero"][k])
            if msg:
                raise GuardError("fill %r changes a result (buffer contents on entry reached it) -- %s" % (tag, msg))
    return res["nan"]
