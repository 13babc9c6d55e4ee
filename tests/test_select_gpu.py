"""Vertex selection on the MI355X (gcn_select_kth / gcn_select_indices / gcn_topk_flag / gcn_race_keys,
pygcn_amd/csrc/gcn_select.hip), `topk_flag` / `sample_without_replacement` / `selection_log_prob` and the fork's
Generator, Hierarchical_Generator and SoftGenerator policy step.

The select and the index rule are held EXACTLY against the numpy restatement tests/_select_ref.py (thresholds as
bit patterns: a NaN threshold is 0x7FC00000 on both sides), a window of a batched call bitwise against the
batch = 1 call on a contiguous copy; the race keys within one fp32 ulp of the restatement (only the last bit of a
double log can differ); the models against the fixture g8_generators.npz with float64 as the arbiter."""
import numpy as np
import pytest
import torch

import _select_ref as R
from conftest import assert_normwise, assert_parity, load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
P8 = np.array([.30, .22, .15, .12, .09, .06, .04, .02], np.float32)


def n_big():
    """The smallest row count whose sweep spans >= 3 blocks with a ragged last one, from the documented formula of
    gcn_select_workspace_bytes (include/gcn_spmm.h): (3 * 2048 + 8 + 2 * B) * 4 bytes for B blocks, block b
    sweeping rows [b * R, min((b + 1) * R, n)), R = ceil(n / B)."""
    from pygcn_amd import _native
    for n in range(1, 1 << 22):
        blocks = (_native.lib().gcn_select_workspace_bytes(n, 1) // 4 - 3 * 2048 - 8) // 2
        rows = -(-n // blocks)
        if blocks >= 3 and (blocks - 1) * rows < n and n % rows != 0:
            return n
    raise AssertionError("no multi-block shape below 2^22 rows")


N_LONG = 1024 * 1024 + 37     # 1024 blocks of 1025 rows (the last one shorter): five 256-row iterations each
SHAPES = ["1", "2", "63", "64", "65", "257", "n_big", "n_long"]


def rows_of(name):
    return {"n_big": n_big, "n_long": lambda: N_LONG}.get(name, lambda: int(name))()


def make_keys(kind, k, n, seed=0):
    """fp32 [k, n], every window different."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "normal":
        return rng.standard_normal((k, n)).astype(np.float32)
    if kind == "low_byte":        # equal in their top 24 bits: the first two digits see ONE bin
        base = np.array([0x3F800000, 0xC0490F00, 0x00000100], np.uint32)[np.arange(k) % 3][:, None]
        return (base | rng.integers(0, 256, (k, n)).astype(np.uint32)).view(np.float32)
    if kind == "all_equal":
        return np.repeat(np.array([1.5, -2.0, 0.0], np.float32)[np.arange(k) % 3][:, None], n, axis=1)
    if kind == "two_values":      # a quarter (at least one) large, the rest small: the ranks n/2 and n fall in the small run
        keys = np.full((k, n), -3.25, np.float32)
        for j in range(k):
            keys[j, rng.permutation(n)[:max(1, n // 4)]] = 7.0 + j
        return keys
    if kind == "special":
        pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000,
                         0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0xBF800000, 0xC2280000, 0x3F800000,
                         0x00800000, 0xFF7FFFFF], np.uint32)
        return pool[rng.integers(0, pool.size, (k, n))].view(np.float32)
    raise AssertionError(kind)


def bits(t):
    return t.view(torch.int32)


def run_select(keys_dev, kth):
    from pygcn_amd.select import kth_largest, topk_indices
    thr, cnt = kth_largest(keys_dev, kth)
    idx = topk_indices(keys_dev, kth, thr, cnt)
    return thr, cnt, idx


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n_name", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "low_byte", "all_equal", "two_values", "special"])
def test_select_equals_the_restatement_exactly(kind, n_name, k):
    n = rows_of(n_name)
    keys = make_keys(kind, k, n)
    dev = torch.from_numpy(keys).to(DEV)
    pre = R.prepared(keys)
    for kth in sorted({1, min(2, n), max(1, n // 2), n}):
        thr, cnt, idx = run_select(dev, kth)
        torch.cuda.synchronize()
        want_thr, want_cnt = R.kth_largest(keys, kth, pre)
        what = f"{kind} [{k}x{n}] kth={kth}"
        assert torch.equal(bits(thr).cpu(), torch.from_numpy(want_thr.view(np.int32))), what
        assert torch.equal(cnt.cpu(), torch.from_numpy(want_cnt)), what
        assert torch.equal(idx.cpu(), torch.from_numpy(R.topk_indices(keys, kth, pre))), what
        if k > 1:
            for j in range(k):
                one = run_select(dev[j:j + 1].contiguous(), kth)
                assert torch.equal(bits(one[0]), bits(thr[j:j + 1])) and torch.equal(one[1], cnt[j:j + 1]), (what, j)
                assert torch.equal(one[2], idx[j:j + 1]), (what, j)


def same_floats(a, b):
    """Bitwise equal, a NaN matching a NaN of any sign or payload (0 * inf is the default NaN of the machine that
    multiplies: negative on x86, positive on gfx950)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def test_flag_kernel_is_numpys_float32_product_under_the_mask():
    from pygcn_amd.functional import topk_flag
    from pygcn_amd.select import flag_above, kth_largest
    k, n = 3, n_big()
    s = make_keys("normal", k, n, seed=1) * np.float32(3.0)
    s[0, :3] = (0.0, np.nan, -np.inf)
    s[0, 3:] = -np.abs(s[0, 3:]) - 1.0               # window 0: the zero is the largest number, so NN = 2 selects it
    s[1, 5] = np.inf
    s[2, 7] = 1e-42                                  # a subnormal score: 1 / s overflows to inf, s * inf = inf
    dev = torch.from_numpy(s).to(DEV)
    for nn_ in (0, 2, n // 3, n - 1):
        thr, _ = kth_largest(dev, nn_ + 1)
        got = flag_above(dev, thr).cpu().numpy()
        want = R.flag(s, R.kth_largest(s, nn_ + 1)[0])
        assert same_floats(got, want), nn_
        assert same_floats(topk_flag(dev, nn_).cpu().numpy(), want), nn_
        if nn_ == 0:
            assert not got.any()                     # nothing selected (the NaN of window 0 is the threshold)
        if nn_ == 2:
            assert np.isnan(got[0, 0]) and got[0, 1] == 0 and got[0, 2] == 0     # 0 * inf; a NaN score is not selected
            assert np.count_nonzero(got[1]) == 2 and np.isnan(got[1, 5])         # inf * 0
    col = torch.from_numpy(s[2]).to(DEV)
    assert same_floats(topk_flag(col.view(n, 1), 5).cpu().numpy().ravel(), R.flag(s[2:3], R.kth_largest(s[2:3], 6)[0])[0])
    assert topk_flag(col, 5).shape == (n,)
    b16 = topk_flag(col.bfloat16(), 5)
    assert b16.dtype == torch.bfloat16 and int((b16 != 0).sum()) <= 5


def test_two_runs_of_every_entry_point_are_bitwise_equal():
    from pygcn_amd.select import flag_above, race_keys
    k, n = 3, n_big()
    p = torch.from_numpy(np.abs(make_keys("normal", k, n, seed=2))).to(DEV)
    runs = []
    for _ in range(2):
        keys = race_keys(p, 99)
        thr, cnt, idx = run_select(keys, 100)
        runs.append((keys, thr, cnt, idx, flag_above(keys, thr)))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    tied = torch.from_numpy(make_keys("low_byte", k, n)).to(DEV)     # many ties at the threshold
    a, b = run_select(tied, n // 2), run_select(tied, n // 2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("seed", [42, (1 << 32) + 12345])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_race_keys_against_the_restatement(n, k, seed):
    from pygcn_amd.select import race_keys
    rng = np.random.default_rng(7)
    p = rng.random((k, n)).astype(np.float32)
    p[:, 3::7] = 0.0
    p[1:] = p[0]                                                     # the same p in every window
    got = race_keys(torch.from_numpy(p).to(DEV), seed).cpu().numpy()
    want = R.race_keys(p, seed)
    assert np.array_equal(want, R.race_keys(p, seed))                # the restatement against itself: none differ
    assert bool((got >= 0).all()) and bool((got[:, 3::7] == 0).all()) and not np.signbit(got).any()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"[{k}x{n}] seed {seed}: max {int(ulps.max())} ulp, {int((ulps != 0).sum())} of {ulps.size} keys differ")
    assert int(ulps.max()) <= 1
    assert int((ulps != 0).sum()) <= 1e-4 * ulps.size
    if n > 1:
        other = race_keys(torch.from_numpy(p).to(DEV), seed + 1).cpu().numpy()
        assert not np.array_equal(other, got)
        if k > 1:
            assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def device_draw_order(keys, nn_):
    """The NN largest of the device's own keys in draw order, by torch: a stable descending sort keeps the lower
    index first on equal keys."""
    return torch.sort(keys, dim=1, descending=True, stable=True).indices[:, :nn_]


@pytest.mark.parametrize("n_name,nn_", [("5", 5), ("257", 1), ("n_big", 100), ("n_big", -1), ("n_long", 1000)])
def test_sample_is_the_top_of_the_devices_own_keys(n_name, nn_):
    from pygcn_amd.functional import sample_without_replacement
    from pygcn_amd.select import race_keys
    k, n = 3, rows_of(n_name)
    nn_ = n if nn_ < 0 else nn_                                      # (-1: every vertex)
    p = np.random.default_rng(8).random((k, n)).astype(np.float32)
    p[1, n // 3:] = 0.0                                              # window 1: two thirds cannot be drawn ...
    dev = torch.from_numpy(p).to(DEV)
    idx = sample_without_replacement(dev, nn_, seed=1234)
    assert idx.shape == (k, nn_) and idx.dtype == torch.int64 and idx.device == dev.device
    assert torch.equal(idx, device_draw_order(race_keys(dev, 1234), nn_))
    got = idx.cpu().numpy()
    for j in range(k):
        assert len(set(got[j].tolist())) == nn_ and got[j].min() >= 0 and got[j].max() < n
    positive = n // 3
    if nn_ > positive:                                               # ... unless NN exceeds the positive ones: then
        assert set(got[1, :positive].tolist()) == set(range(positive))            # all of those first,
        assert got[1, positive:].tolist() == list(range(positive, nn_))           # and zeros by lowest index
    else:
        assert got[1].max() < positive
    one = sample_without_replacement(dev[0], nn_, seed=1234)
    assert one.shape == (nn_,) and torch.equal(one, idx[0])


def test_sample_has_the_law_of_draws_without_replacement():
    """The CPU test's statistics on the device's picks, with the same bounds."""
    from pygcn_amd.functional import sample_without_replacement
    idx = sample_without_replacement(torch.from_numpy(np.tile(P8, (4096, 1))).to(DEV), 2, seed=42).cpu().numpy()
    z1, z2 = R.race_statistics(idx[:, 0], idx[:, 1], P8)
    print(f"first pick: max {z1:.2f} sigma; ordered pair: max {z2:.2f} sigma")
    assert z1 <= 4.0 and z2 <= 4.5


def test_sample_follows_torch_manual_seed():
    from pygcn_amd.functional import sample_without_replacement
    p = torch.from_numpy(np.random.default_rng(9).random((2, 5000)).astype(np.float32)).to(DEV)
    torch.manual_seed(5)
    a1, a2 = sample_without_replacement(p, 50), sample_without_replacement(p, 50)
    torch.manual_seed(5)
    b1, b2 = sample_without_replacement(p, 50), sample_without_replacement(p, 50)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)


# ---------------------------------------------------------------------------- gradients, host synchronisation
def test_topk_flag_gradient_against_float64():
    """d flag / d s = (s > t ? 1 / s : 0): one fp32 reciprocal and one product, each rounded once, so 2^-23 of
    the float64 value elementwise; held at 2^-22 of max|gradient|."""
    from pygcn_amd.functional import topk_flag
    k, n, nn_ = 3, n_big(), 40
    s = torch.from_numpy(make_keys("normal", k, n, seed=3))
    g = torch.from_numpy(make_keys("normal", k, n, seed=4))
    sd = s.to(DEV).requires_grad_()
    out = topk_flag(sd, nn_)
    assert out.grad_fn.name().startswith("TopkFlagFunction")
    out.backward(g.to(DEV))
    for j in range(k):
        s64 = s[j].double().view(n, 1).requires_grad_()
        R.literal_flag(s64, nn_).backward(g[j].double().view(n, 1))
        assert_normwise(sd.grad[j].cpu().numpy(), s64.grad.view(n).numpy(), rel=2.0 ** -22, what=f"flag gradient, row {j}")
        assert int((sd.grad[j] != 0).sum()) == nn_
    col = s[0].view(n, 1).to(DEV).requires_grad_()
    topk_flag(col, nn_).backward(g[0].view(n, 1).to(DEV))
    assert torch.equal(col.grad.view(n), sd.grad[0])


def test_selection_log_prob_against_categorical_in_float64():
    from pygcn_amd.functional import selection_log_prob
    rng = np.random.default_rng(10)
    w = torch.from_numpy((rng.random((3, 5000)) + 1e-3).astype(np.float32))
    idx = torch.from_numpy(np.stack([rng.permutation(5000)[:50] for _ in range(3)]))
    p = w.to(DEV).requires_grad_()
    got = selection_log_prob(p, idx.to(DEV))
    got.sum().backward()
    p64 = w.double().requires_grad_()
    want = torch.stack([torch.distributions.Categorical(p64[j]).log_prob(idx[j]).sum() for j in range(3)])
    want.sum().backward()
    assert got.shape == (3,) and got.dtype == torch.float32
    assert_normwise(got.detach().cpu().numpy(), want.detach().numpy(), rel=1e-6, what="log-prob on the device")
    assert_normwise(p.grad.cpu().numpy(), p64.grad.numpy(), rel=1e-5, what="log-prob gradient on the device")


def count_host_syncs(fn):
    """Host synchronisations of one call of `fn`, counted the way bench.py counts host_syncs_per_step: torch's
    sync debug mode and hooks on .item() / .tolist() / .cpu() / torch.nonzero, the larger count; the detectors must
    see a deliberate .item() first."""
    import warnings

    def run(call):
        seen, hooks = [], []
        for name in ("item", "tolist", "cpu"):
            real = getattr(torch.Tensor, name)
            hooks.append((torch.Tensor, name, real))
            setattr(torch.Tensor, name, (lambda r, nm: lambda t, *a, **kw: (
                seen.append(nm) if t.is_cuda else None, r(t, *a, **kw))[1])(real, name))
        real_nz = torch.nonzero
        hooks.append((torch, "nonzero", real_nz))
        torch.nonzero = lambda *a, **kw: (seen.append("nonzero"), real_nz(*a, **kw))[1]
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                call()
            warned = sum("synchroniz" in str(w.message).lower() for w in caught)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            while hooks:
                obj, name, real = hooks.pop()
                setattr(obj, name, real)
        return max(warned, len(seen))
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    assert run(lambda: probe.item()) >= 1, "the detectors did not see a deliberate .item()"
    n_sync = run(fn)
    torch.cuda.synchronize()
    return n_sync


def g7_model():
    import _attention_ref as A
    from pygcn_amd import CSRGraph, SoftGenerator
    g7 = load_golden("g7_soft_generator.npz")
    state, x, adj, d, picked, reward = A.fixture_case(g7)
    dims = [int(v) for v in g7["dims"]]
    model = SoftGenerator(dims[0], dims[1], dims[2], 0.0, dims[5], dims[3], dims[4], dim_touched=d)
    model.load_state_dict(state, strict=True)
    n = x.shape[0]
    graph = CSRGraph(torch.from_numpy(g7["rowptr"]).to(DEV), torch.from_numpy(g7["col"]).to(DEV),
                     torch.from_numpy(g7["val"]).to(DEV), (n, n))
    return model.to(DEV).train(), x.to(DEV), graph, dims[5]


def test_no_host_synchronisation():
    from pygcn_amd.functional import sample_without_replacement, topk_flag
    s = torch.from_numpy(make_keys("normal", 3, n_big(), seed=5)).to(DEV).requires_grad_()
    p = torch.rand(3, n_big(), device=DEV)
    model, x, graph, _ = g7_model()
    model.select_action(x, graph)                        # (first use builds the graph's plans,
    model.saved_log_probs[-1].backward()                 #  the first backward pass those of its transpose)
    torch.manual_seed(1)

    def flag_step():
        topk_flag(s, 50).sum().backward()

    assert count_host_syncs(flag_step) == 0
    assert count_host_syncs(lambda: sample_without_replacement(p, 50)) == 0
    assert count_host_syncs(lambda: sample_without_replacement(p, 50, seed=3)) == 0
    assert count_host_syncs(lambda: model.select_action(x, graph)) == 0
    assert count_host_syncs(lambda: model.saved_log_probs[-1].backward()) == 0


# ------------------------------------------------------------------------------------------------- models
class LaunchSpy:
    """Records (name, args) of every _native.launch while it forwards them."""

    def __init__(self, monkeypatch):
        from pygcn_amd import _native
        self.calls, real = [], _native.launch

        def launch(name, device, *args, **kw):
            self.calls.append((name, args))
            return real(name, device, *args, **kw)
        monkeypatch.setattr(_native, "launch", launch)

    def names(self):
        return [name for name, _ in self.calls]


@pytest.mark.parametrize("tag", ["gen_", "hier_"])
def test_generators_against_the_fixture(monkeypatch, tag):
    """The fixture's model on the device: scores and every parameter gradient of vac_flag.sum() against the
    reference's own run with float64 from the restatement as the arbiter; the flag exactly (the chosen set is the
    fixture's, the values are the model's own s * (1 / s), _select_ref.assert_flag_exact)."""
    import pygcn_amd
    from pygcn_amd import CSRGraph
    from pygcn_amd.sharded import ShardedGraph
    g8 = load_golden("g8_generators.npz")
    hier = tag == "hier_"
    state, x, adj, d, nn_ = R.fixture_case(g8, tag)
    dims = [int(v) for v in g8["dims"]]
    cls = pygcn_amd.Hierarchical_Generator if hier else pygcn_amd.Generator
    model = cls(dims[0], dims[1], dims[2], 0.0, nn_, dims[2] + x.shape[1] - d - hier, dims[3], dims[4], dim_touched=d)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    n = x.shape[0]
    graph = CSRGraph(torch.from_numpy(g8["rowptr"]).to(DEV), torch.from_numpy(g8["col"]).to(DEV),
                     torch.from_numpy(g8["val"]).to(DEV), (n, n))
    spy = LaunchSpy(monkeypatch)
    scores = model.scores(x.to(DEV), graph)
    flag = model(x.to(DEV), graph)
    flag.sum().backward()
    torch.cuda.synchronize()
    wanted = ["gcn_select_kth", "gcn_topk_flag"] + ([] if hier else ["gcn_bn_stats_batched", "gcn_bn_apply_batched",
                                                                     "gcn_bn_backward_sums_batched",
                                                                     "gcn_bn_backward_apply_batched"])
    for name in wanted:
        assert name in spy.names(), (name, spy.names())
    assert flag.shape == (n, 1) and flag.dtype == torch.float32
    s64, f64, g64 = R.generator_step(state, x, adj, d, nn_, torch.float64, hier)
    assert_parity(scores.detach().cpu().numpy(), g8[tag + "scores"], s64, tag + "scores")
    R.assert_flag_exact(flag.detach().cpu().numpy(), scores.detach().cpu().numpy(), g8[tag + "vac_flag"], nn_, tag + "flag")
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(state)
    for name in state:
        assert_parity(params[name].grad.cpu().numpy(), g8[tag + "grad_" + name], g64[name], f"{tag}grad {name}")
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        model(x.to(DEV), object.__new__(ShardedGraph))


def test_soft_generator_policy_step():
    g8 = load_golden("g8_generators.npz")
    model, x, graph, nn_ = g7_model()
    picked = torch.from_numpy(g8["g7_picked"])
    lp = model.log_prob(x, graph, picked.to(DEV))
    assert_normwise(float(lp.detach()), float(g8["g7_log_prob"].reshape(())), rel=1e-5, what="SoftGenerator.log_prob vs g8")
    assert float(model.log_prob(x, graph, picked.tolist()).detach()) == float(lp.detach())
    before = model(x, graph).detach()
    vac_flag, idx = model.select_action(x, graph, seed=77)
    assert vac_flag.shape == before.shape and idx.shape == (nn_,) and idx.dtype == torch.int64 and idx.is_cuda
    want = torch.zeros_like(before)
    want[idx] = 1.0
    assert torch.equal(vac_flag, want) and int(vac_flag.sum()) == nn_ and not vac_flag.requires_grad
    again = model.select_action(x, graph, seed=77)
    assert torch.equal(again[1], idx) and len(model.saved_log_probs) == 2
    assert torch.equal(model.saved_log_probs[0].detach(), model.saved_log_probs[1].detach())
    assert_normwise(float(model.saved_log_probs[0].detach()), float(model.log_prob(x, graph, idx).detach()), rel=1e-6,
                    what="the appended log-probability is log_prob of the picks")
    (-0.7 * model.saved_log_probs[0]).backward()
    torch.cuda.synchronize()
    for name, prm in model.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0, name


# -------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every bad call returns its code before a launch
    and names itself in gcn_last_error()."""
    from pygcn_amd import _native
    L = _native.lib()
    n, k, m = 37, 3, 5
    keys = torch.rand(k, n + 1, device=DEV)
    out = torch.zeros(k, n + 1, device=DEV)
    thr = torch.zeros(k + 1, device=DEV)
    cnt = torch.zeros(k + 1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(k * m + 1, dtype=torch.int64, device=DEV)
    need = L.gcn_select_workspace_bytes(n, k)
    assert need == k * (3 * 2048 + 8 + 2) * 4
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    seed = torch.tensor([42, 0], dtype=torch.int64, device=DEV)
    kp, op, tp, cp, ip, wp, sp = (t.data_ptr() for t in (keys, out, thr, cnt, idx, ws, seed))

    def calls(n=n, k=k, m=m, kp=kp, tp=tp, ip=ip, wp=wp, need=need, sp=sp):
        return {
            "gcn_select_kth": lambda: L.gcn_select_kth(kp, n, k, m, tp, cp, wp, need, None),
            "gcn_select_indices": lambda: L.gcn_select_indices(kp, n, k, m, tp, cp, ip, wp, need, None),
            "gcn_topk_flag": lambda: L.gcn_topk_flag(kp, n, k, tp, op, None),
            "gcn_race_keys": lambda: L.gcn_race_keys(kp, n, k, 42, op, None),
            "gcn_race_keys_dev": lambda: L.gcn_race_keys_dev(kp, n, k, sp, op, None),
        }

    def expect(table, code, only=None):
        for name, call in table.items():
            if only is None or name in only:
                assert call() == code, name
                if code != 0:
                    assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    ranked = ("gcn_select_kth", "gcn_select_indices")
    expect(calls(n=0), -1)                       # GCN_E_BADARG: n_rows, batch, kth / m out of range
    expect(calls(n=1 << 31), -1)
    expect(calls(k=0), -1)
    expect(calls(k=65536), -1)
    expect(calls(m=0), -1, ranked)
    expect(calls(m=n + 1), -1, ranked)
    expect(calls(kp=None), -1)                   # GCN_E_BADARG: NULL tensor
    expect(calls(tp=None), -1, ranked + ("gcn_topk_flag",))
    expect(calls(ip=None), -1, ("gcn_select_indices",))
    expect(calls(sp=None), -1, ("gcn_race_keys_dev",))   # the device seed is not optional
    expect(calls(kp=kp + 2), -2)                 # GCN_E_ALIGN: a float off the 4-byte grid
    expect(calls(ip=ip + 4), -2, ("gcn_select_indices",))
    expect(calls(sp=sp + 4), -2, ("gcn_race_keys_dev",))  # a 64-bit seed off the 8-byte grid
    expect(calls(wp=wp + 1), -2, ranked)
    expect(calls(need=need - 1), -3, ranked)     # GCN_E_WORKSPACE: one byte short, or NULL
    expect(calls(wp=None), -3, ranked)
    expect(calls(), 0)                           # and the good calls launch
    torch.cuda.synchronize()
