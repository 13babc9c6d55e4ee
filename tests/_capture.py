"""hipGraph capture and replay for the tests (tests/test_capture_gpu.py): torch's documented recipe, one stream, no
parallel branches, no environment variable set or read.

  capture(fn)        three eager warm-up calls of `fn` on one side stream, wait_stream, then `fn` captured with
                     torch.cuda.CUDAGraph() under torch.cuda.graph(...): a Captured of the graph and fn's static
                     outputs.  A host read, an allocation outside the graph's pool or a launch on another stream
                     makes torch raise during the capture, and that is the detector.
  Captured.replay()  fills every static output with NaN (integers: their lowest value) and replays: a launch that
                     is missing from the graph shows up as NaN instead of as the warm-up's leftover result — the
                     idea of the `poison` fixture of tests/test_fused_gpu.py.
  spy                a LaunchSpy of tests/test_select_gpu.py: the C-ABI entry points launched DURING the capture
                     (warm-up and eager calls excluded) are left in Captured.launched.
"""
import torch


def tensors_of(out):
    """The tensors of a result, in order: a tensor, None, or nested tuples / lists / dicts of them; an object with
    `slots` and `dense` (spmm.PackedRows) counts as that pair."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in out for t in tensors_of(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors_of(o)]
    if hasattr(out, "slots") and hasattr(out, "dense"):
        return [out.slots]
    raise TypeError(f"no tensors in a {type(out).__name__}")


def snapshot(out):
    """Clones of the tensors of a result, taken on the current stream, as plain tensors."""
    return [t.detach().as_subclass(torch.Tensor).clone() for t in tensors_of(out)]


def poison_(t):
    t = t.detach().as_subclass(torch.Tensor)
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(torch.iinfo(t.dtype).min)


class Captured:
    def __init__(self, graph, outputs, launched):
        self.graph, self.outputs, self.launched = graph, outputs, launched

    def replay(self, poison=True):
        """One replay; returns clones of the static outputs."""
        if poison:
            for t in tensors_of(self.outputs):
                poison_(t)
        self.graph.replay()
        return snapshot(self.outputs)


def capture(fn, spy=None, warmup=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    before = len(spy.calls) if spy is not None else 0
    with torch.cuda.graph(graph):
        outputs = fn()
    launched = [name for name, _ in spy.calls[before:]] if spy is not None else []
    return Captured(graph, outputs, launched)


def bits_equal(a, b):
    """Same shape, dtype and bytes (a NaN equals the same NaN; +0 differs from -0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
    return bool(torch.equal(a, b))


def assert_bitwise(got, want, what):
    """Two snapshots, tensor by tensor; names the first differing tensor, how many elements differ and whether the
    replay left poison behind (a launch missing from the graph)."""
    assert len(got) == len(want), f"{what}: {len(got)} outputs against {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if bits_equal(g, w):
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {i} is {tuple(g.shape)} {g.dtype}, " \
                                                          f"eager gives {tuple(w.shape)} {w.dtype}"
        differ = int((g != w).sum()) if not g.dtype.is_floating_point else \
            int(((g != w) & ~(torch.isnan(g) & torch.isnan(w))).sum())
        nans = int(torch.isnan(g).sum()) if g.dtype.is_floating_point else 0
        err = float((g.double() - w.double()).abs().nan_to_num(float("inf")).max()) if g.numel() else 0.0
        raise AssertionError(f"{what}: output {i} {tuple(g.shape)} {g.dtype}: {differ} of {g.numel()} elements differ "
                             f"from the eager call, max |d| = {err:.3e}, {nans} NaN in the replay's output")


def any_differs(a, b):
    return any(not bits_equal(x, y) for x, y in zip(a, b))
