"""The evaluator GCN_OVER_MLP on the MI355X: the two ingest sweeps (gcn_eval_ingest / gcn_eval_ingest_backward,
pygcn_amd/csrc/gcn_eval.hip) against numpy, `masked_mean_pool(mask_grad=True)`, and the model
(pygcn_amd.models.GCN_OVER_MLP; reference pygcn/models.py:333-355) against the restatement of the fork's lines
(tests/_evaluator_ref.py) on the CPU — float64 the arbiter, float32 the reference arithmetic, both through
conftest.assert_parity at the project's 1e-5 — and against the fixture g9_evaluator.npz.

Copies (`wide`, `mask`, the columns of dx below dim_touched) are held BITWISE; the masked sums against the
float64 sum of the exactly representable products within a double-summation bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _evaluator_ref as R
import test_batched_norm_gpu as B
import test_norm_gpu as T
import test_select_gpu as S
from conftest import assert_normwise, assert_parity, load_golden
from test_evaluator_cpu import KEYS, g9_case
from test_norm_gpu import DEV, seeded

pytestmark = pytest.mark.gpu


def n_big(k, f, d):
    """The smallest row count whose sweep spans >= 3 blocks with a ragged last one, from the documented formula
    of gcn_eval_workspace_bytes (include/gcn_spmm.h): B * batch * (F - d) * sizeof(double) bytes for B blocks,
    block b sweeping rows [b * R, min((b + 1) * R, n)), R = 64 * ceil(n / (64 * B)), in tiles of 64 — so a
    retune of the slab size moves this shape with it."""
    from pygcn_amd import _native
    for n in range(1, 1 << 22):
        blocks = _native.lib().gcn_eval_workspace_bytes(n, f, d, k) // (k * (f - d) * 8)
        rows = 64 * -(-n // (64 * blocks))
        if blocks >= 3 and (blocks - 1) * rows < n and n % rows != 0:
            return n
    raise AssertionError("no multi-block shape below 2^22 rows")


def n_two_tiles(k, f, d):
    """The smallest row count at which a block sweeps more than one tile of 64 rows (its sums then run over
    tiles, the LDS image is reused) with a ragged last tile; blocks past the last row sweep nothing."""
    from pygcn_amd import _native
    cap = _native.lib().gcn_eval_workspace_bytes(1 << 40, f, d, k) // (k * (f - d) * 8)      # the block cap
    return 64 * cap + 64 + 5


SHAPES = [(1, "1", 2, 1), (1, "37", 9, 8), (3, "37", 17, 8), (3, "37", 5, 0), (2, "37", 64, 31), (20, "n_big", 9, 8),
          (5, "n_big", 17, 8), (2, "two_tiles", 9, 8), (3, "two_tiles", 6, 2)]


def rows_of(name, k, f, d):
    return n_big(k, f, d) if name == "n_big" else n_two_tiles(k, f, d) if name == "two_tiles" else int(name)


def inputs(k, n, f, with_flag, seed=7):
    """x with a Bernoulli 0/1 flag as its last column — when a separate flag is given, the last column of x is
    standard normal instead: it must not be read."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((k, n, f)).astype(np.float32)
    flag = (rng.random((k, n)) < 0.3).astype(np.float32)
    if with_flag:
        return x, flag
    x[:, :, -1] = flag
    return x, None


def dev(a):
    return torch.from_numpy(a).to(DEV) if a is not None else None


def bits(t):
    """The tensor as integers of its width: equality that holds for NaNs too."""
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


# ------------------------------------------------------------------------------------------ ingest forward
@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("k,n_name,f,d", SHAPES)
def test_ingest_forward_against_numpy(k, n_name, f, d, with_flag):
    from pygcn_amd.evaluator import ingest
    n = rows_of(n_name, k, f, d)
    x, flag = inputs(k, n, f, with_flag)
    wide, mask, esum, nonzero = ingest(dev(x), d, dev(flag))
    again = ingest(dev(x), d, dev(flag))
    torch.cuda.synchronize()
    m = flag if with_flag else x[:, :, -1]
    e = f - 1 - d
    assert wide.shape == (n, k * d) and mask.shape == (k, n) and esum.shape == (k * e,) and nonzero.shape == (k,)
    assert esum.dtype == torch.float64 and nonzero.dtype == torch.int64
    assert np.array_equal(wide.cpu().numpy(), x[:, :, :d].transpose(1, 0, 2).reshape(n, k * d))      # copies: bitwise
    assert np.array_equal(mask.cpu().numpy(), m)
    assert np.array_equal(nonzero.cpu().numpy(), (m != 0).sum(1))
    terms = m.astype(np.float64)[:, :, None] * x[:, :, d:f - 1].astype(np.float64)       # exact in double
    ref, bound = terms.sum(1), n * 2.0 ** -52 * np.abs(terms).sum(1)
    gap = np.abs(esum.cpu().numpy().reshape(k, e) - ref)
    print(f"esum [{k}x{n}x{f}, d={d}]: max gap / bound = {float((gap / np.maximum(bound, 1e-300)).max()) if e else 0.0:.3g}")
    assert (gap <= bound).all()
    for a, b in zip((wide, mask, esum, nonzero), again):                                  # reproducible: bitwise
        assert torch.equal(a, b)


def test_ingest_nan_and_skipped_outputs():
    """A NaN in one sample's untouched column poisons only that sample's column sum; a zero flag over a NaN gives
    NaN (the mask multiplies); a NaN flag counts as non-zero; NULL output pointers skip their output."""
    from pygcn_amd import _native
    from pygcn_amd.evaluator import ingest
    k, f, d = 3, 17, 8
    n = n_big(k, f, d)
    e = f - 1 - d
    x, _ = inputs(k, n, f, False, seed=9)
    row = int(np.flatnonzero(x[1, :, -1] == 0)[0])          # a vertex of sample 1 whose flag is 0
    x[1, row, d + 2] = np.nan
    x[2, 5, -1] = np.nan                                    # a NaN flag: counts, and poisons all of sample 2's sums
    _, mask, esum, nonzero = ingest(dev(x), d)
    got = np.isnan(esum.cpu().numpy().reshape(k, e))
    want = np.zeros((k, e), bool)
    want[1, 2] = True
    want[2, :] = True
    assert np.array_equal(got, want)
    assert np.array_equal(nonzero.cpu().numpy(), (x[:, :, -1] != 0).sum(1)) and np.isnan(x[2, 5, -1])
    # every output on its own: the same bits, the others untouched
    xd = dev(x)
    wide_all, mask_all, esum_all, nz_all = ingest(xd, d)
    L = _native.lib()
    need = L.gcn_eval_workspace_bytes(n, f, d, k)
    for which in range(4):
        outs = [torch.full((n, k * d), -7.0, device=DEV), torch.full((k, n), -7.0, device=DEV),
                torch.full((k * e,), -7.0, dtype=torch.float64, device=DEV),
                torch.full((k,), -7, dtype=torch.int64, device=DEV)]
        ptrs = [o.data_ptr() if i == which else None for i, o in enumerate(outs)]
        _native.launch("gcn_eval_ingest", DEV, xd.data_ptr(), None, n, f, d, k, *ptrs, workspace=need)
        torch.cuda.synchronize()
        for i, (o, full) in enumerate(zip(outs, (wide_all, mask_all, esum_all, nz_all))):
            if i == which:
                assert torch.equal(bits(o), bits(full)), i
            else:
                assert bool((o == -7).all()), (which, i)


# ----------------------------------------------------------------------------------------- ingest backward
@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("k,n_name,f,d", SHAPES)
def test_ingest_backward_against_numpy(k, n_name, f, d, with_flag):
    from pygcn_amd.evaluator import ingest_backward
    n = rows_of(n_name, k, f, d)
    e = f - 1 - d
    x, flag = inputs(k, n, f, with_flag, seed=11)
    rng = np.random.default_rng(12)
    d_wide = rng.standard_normal((n, k * d)).astype(np.float32)
    d_mask = rng.standard_normal((k, n)).astype(np.float32)
    d_esum = rng.standard_normal((k, e)).astype(np.float32)
    m = flag if with_flag else x[:, :, -1]
    xd, fd = dev(x), dev(flag)

    def run(gw, gm, ge, need_dx=True):
        dx, dflag = ingest_backward(xd, d, fd, dev(gw), dev(gm), dev(ge), need_dx, with_flag)
        torch.cuda.synchronize()
        return (dx.cpu().numpy() if dx is not None else None), (dflag.cpu().numpy() if dflag is not None else None)

    def check(dx, dflag, gw, gm, ge, what):
        zw, zm, ze = np.zeros_like(d_wide), np.zeros_like(d_mask), np.zeros_like(d_esum)
        gw, gm, ge = (gw if gw is not None else zw), (gm if gm is not None else zm), (ge if ge is not None else ze)
        if dx is not None:
            assert dx.shape == (k, n, f)
            assert np.array_equal(dx[:, :, :d], gw.reshape(n, k, d).transpose(1, 0, 2)), what      # bitwise
            prod = (torch.from_numpy(m)[:, :, None] * torch.from_numpy(ge)[:, None, :]).numpy()      # torch's fp32 product
            if ge is ze:
                prod = np.zeros_like(prod)                  # (a NULL gradient is zero, whatever the mask)
            assert np.array_equal(dx[:, :, d:f - 1], prod), what
        terms = x[:, :, d:f - 1].astype(np.float64) * ge.astype(np.float64)[:, None, :]
        ref = gm.astype(np.float64) + (terms.sum(2) if ge is not ze else 0.0)
        bound = 2.0 ** -23 * np.abs(ref) + n * 2.0 ** -52 * (np.abs(terms).sum(2) + np.abs(gm))
        dm = dflag if with_flag else dx[:, :, -1]
        assert (np.abs(dm - ref) <= bound).all(), what
        if with_flag and dx is not None:
            assert not dx[:, :, -1].any(), what

    full = run(d_wide, d_mask, d_esum)
    check(*full, d_wide, d_mask, d_esum, "all gradients")
    for gw, gm, ge, what in ((None, d_mask, d_esum, "d_wide NULL"), (d_wide, None, d_esum, "d_mask NULL"),
                             (d_wide, d_mask, None, "d_esum NULL"), (None, None, None, "all NULL")):
        check(*run(gw, gm, ge), gw, gm, ge, what)
    if with_flag:                       # only the flag's gradient: the same bits, nothing else written
        dx, dflag = run(None, d_mask, d_esum, need_dx=False)
        assert dx is None and np.array_equal(dflag, full[1])


# --------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every call returns before a launch."""
    from pygcn_amd import _native
    L = _native.lib()
    k, n, f, d = 3, 37, 17, 8
    e = f - 1 - d
    x = torch.randn(k, n, f, device=DEV)
    flag, wide, mask = torch.ones(k, n, device=DEV), torch.zeros(n, k * d, device=DEV), torch.zeros(k, n, device=DEV)
    esum, nz = torch.zeros(k * e, dtype=torch.float64, device=DEV), torch.zeros(k, dtype=torch.int64, device=DEV)
    de, dx = torch.zeros(k * e, device=DEV), torch.zeros(k, n, f, device=DEV)
    need = L.gcn_eval_workspace_bytes(n, f, d, k)
    assert need == 1 * k * (f - d) * 8
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    xp, fp, wp = x.data_ptr(), flag.data_ptr(), ws.data_ptr()

    def calls(n=n, f=f, d=d, k=k, xp=xp, fp=fp, wsp=wp, need=need, esp=esum.data_ptr(), dxp=dx.data_ptr(), dfp=None):
        return {
            "gcn_eval_ingest": lambda: L.gcn_eval_ingest(xp, fp, n, f, d, k, wide.data_ptr(), mask.data_ptr(), esp,
                                                         nz.data_ptr(), wsp, need, None),
            "gcn_eval_ingest_backward": lambda: L.gcn_eval_ingest_backward(xp, fp, wide.data_ptr(), mask.data_ptr(),
                                                                           de.data_ptr(), n, f, d, k, dxp, dfp, None),
        }

    def expect(table, code, only=None):
        for name, call in table.items():
            if only is None or name in only:
                assert call() == code, name
                assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    for bad in (dict(n=0), dict(f=1), dict(f=65), dict(d=-1), dict(d=f), dict(k=0), dict(k=65536), dict(xp=None)):
        expect(calls(**bad), -1)                                       # GCN_E_BADARG
    expect(calls(fp=None, dxp=None, dfp=mask.data_ptr()), -1, ["gcn_eval_ingest_backward"])   # dflag without flag
    expect(calls(dxp=None), -1, ["gcn_eval_ingest_backward"])          # neither dx nor dflag
    expect(calls(xp=xp + 2), -2)                                       # GCN_E_ALIGN: a misaligned base pointer
    expect(calls(fp=fp + 2), -2)
    expect(calls(esp=esum.data_ptr() + 4), -2, ["gcn_eval_ingest"])
    expect(calls(dxp=dx.data_ptr() + 1), -2, ["gcn_eval_ingest_backward"])
    expect(calls(wsp=wp + 8), -2, ["gcn_eval_ingest"])
    expect(calls(need=need - 1), -3, ["gcn_eval_ingest"])              # GCN_E_WORKSPACE: one byte short
    expect(calls(wsp=None), -3, ["gcn_eval_ingest"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the pool's mask gradient
@pytest.mark.parametrize("k,c,n_name", [(1, 16, "37"), (3, 32, "37"), (3, 32, "n_big"), (2, 256, "n_big")])
def test_masked_mean_pool_mask_gradient(k, c, n_name):
    from pygcn_amd.functional import masked_mean_pool
    n = T.rows_of(n_name, c)
    h, cot = seeded((k, n, c), 141), seeded((k, c), 142)
    mask = B.bernoulli_mask(k, n, 143)
    mask[:, 0] = 1.0
    count = (mask[0] != 0).sum()
    hd, md = B.wide_view(h).requires_grad_(), mask.to(DEV).requires_grad_()
    out = masked_mean_pool(hd, md, count=count.to(DEV), mask_grad=True)
    assert out.grad_fn.name().startswith("MaskedMeanPoolFunction"), out.grad_fn.name()
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()

    def ref(dtype):
        hh, mm = h.clone().to(dtype).requires_grad_(), mask.clone().to(dtype).requires_grad_()
        o = (hh * mm[:, :, None]).sum(1) / count.to(dtype)
        o.backward(cot.to(dtype))
        return o.detach().numpy(), hh.grad.numpy(), mm.grad.numpy()
    r32, r64 = ref(torch.float32), ref(torch.float64)
    for name, a, a32, a64 in zip(("pooled", "dh", "dmask"), (out.detach(), hd.grad, md.grad), r32, r64):
        assert a.dtype == torch.float32
        assert_parity(a.cpu().numpy(), a32, a64, f"{name} [{k}x{n}x{c}]")
    # the default is the call from before the keyword existed: the same bits, and no gradient for the mask
    h0, h1 = hd.detach().requires_grad_(), hd.detach().requires_grad_()
    m0 = md.detach().requires_grad_()
    old, new = masked_mean_pool(h0, m0, count.to(DEV)), masked_mean_pool(h1, m0, count.to(DEV), mask_grad=False)
    old.backward(cot.to(DEV))
    new.backward(cot.to(DEV))
    assert torch.equal(old, new) and torch.equal(old, out.detach()) and torch.equal(h0.grad, h1.grad)
    assert torch.equal(h0.grad, hd.grad) and m0.grad is None


# ------------------------------------------------------------------------------------------------ the model
def evaluator(f, seed=42):
    from pygcn_amd import GCN_OVER_MLP
    torch.manual_seed(seed)
    model = GCN_OVER_MLP(8, 32, 32, 0.5, 3, 32 + f - 1 - 8, 16, 8, dim_touched=8)
    state = {name: v.detach().clone() for name, v in model.state_dict().items()}
    return model.to(DEV).train(), state


def model_input(k, n, f, seed):
    x = seeded((k, n, f), seed)
    x[:, :, -1] = B.bernoulli_mask(k, n, seed + 1)
    return x


def parent_route(model, x, adj, d):
    """The same evaluator written only with what existed before GCN_OVER_MLP: GCNBatchNorm on x[:, :, :d],
    torch.cat, the fork's pool lines (reference pygcn/models.py:351, :272, :279) and MLPLayers."""
    h = model.GCNLayer(x[:, :, :d].contiguous(), adj)
    return model.MLPLayers(R.pool_layer(torch.cat((h, x[:, :, d:]), dim=2)))


@pytest.mark.parametrize("k,f", [(3, 17), (3, 9), (1, 17)])
@pytest.mark.parametrize("case", list(B.CASES))
def test_model_step_matches_the_fork_on_the_cpu(case, k, f):
    n, edges = B.CASES[case][:2]
    adj_cpu, adj_dev = B._graph(n, edges)
    model, state = evaluator(f)
    x, target = model_input(k, n, f, 151), seeded((k, 1), 153)
    xd = x.to(DEV).requires_grad_()
    out = model(xd, adj_dev)
    assert out.shape == (k, 1)
    F.mse_loss(out, target.to(DEV)).backward()
    masks = B.batched_relu_masks(model.GCNLayer, xd[:, :, :8], adj_dev)
    torch.cuda.synchronize()
    gcn_state = {name[len("GCNLayer."):]: v for name, v in state.items() if name.startswith("GCNLayer.")}
    for j in range(k):
        T.check_relu_masks(masks[j], gcn_state, x[j, :, :8], adj_cpu)
    loss = lambda o: F.mse_loss(o, target.to(o.dtype))      # noqa: E731
    o32, g32, f32 = R.evaluator_step(state, x, adj_cpu, 8, torch.float32, loss, masks)
    o64, g64, f64 = R.evaluator_step(state, x, adj_cpu, 8, torch.float64, loss, masks)
    what = f"{case}, k={k}, F={f}"
    assert_parity(out.detach().cpu().numpy(), o32, o64, f"{what}: output")
    assert_parity(xd.grad[:, :, -1].cpu().numpy(), f32, f64, f"{what}: x.grad[:, :, -1]")
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(KEYS)
    for name in KEYS:
        assert_parity(params[name].grad.cpu().numpy(), g32[name], g64[name], f"{what}: {name}.grad")


@pytest.mark.parametrize("k,f", [(3, 17), (1, 9)])
def test_flag_inside_x_flag_on_its_own_and_the_parent_route_agree(k, f):
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    model, _ = evaluator(f)
    x, target = model_input(k, n, f, 161).to(DEV), seeded((k, 1), 163).to(DEV)
    results = []
    for route in ("inside", "own", "parent"):
        model.zero_grad()
        flag = x[:, :, -1].clone().requires_grad_()
        if route == "own":
            data = x.clone()
            data[:, :, -1] = 123.0                                  # any last column: it is not read
            out = model(data, adj_dev, flag=flag)
        else:
            xin = torch.cat((x[:, :, :-1], flag.unsqueeze(2)), dim=2)
            out = model(xin, adj_dev) if route == "inside" else parent_route(model, xin, adj_dev, 8)
        F.mse_loss(out, target).backward()
        results.append((out.detach().cpu().numpy(), flag.grad.cpu().numpy(),
                        {name: p.grad.cpu().numpy() for name, p in model.named_parameters()}))
    torch.cuda.synchronize()
    for name, got in zip(("flag inside x", "flag on its own"), results[:2]):
        assert_normwise(got[0], results[2][0], what=f"{name} vs the parent route: output")
        assert_normwise(got[1], results[2][1], what=f"{name} vs the parent route: flag gradient")
        for p in KEYS:
            assert_normwise(got[2][p], results[2][2][p], what=f"{name} vs the parent route: {p}.grad")
    assert_normwise(results[1][0], results[0][0], what="own vs inside: output")
    assert_normwise(results[1][1], results[0][1], what="own vs inside: flag gradient")
    if k == 1:      # the shapes Generator returns
        for shape in ((n,), (n, 1)):
            flag = x[:, :, -1].clone().reshape(shape).requires_grad_()
            out = model(x, adj_dev, flag=flag)
            F.mse_loss(out, target).backward()
            assert flag.grad.shape == shape
            assert_normwise(flag.grad.reshape(1, n).cpu().numpy(), results[1][1], what=f"flag {shape}")


def test_generator_trains_through_the_evaluator():
    """flag = Generator(x_gen, adj); loss = evaluator(feats, adj, flag=flag); loss.backward() (reference
    pygcn/policy-generator.py:398-420): every Generator parameter's gradient against the same chain through
    torch.cat."""
    from pygcn_amd import Generator
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    f = 17
    model, _ = evaluator(f)
    torch.manual_seed(7)
    gen = Generator(8, 32, 32, 0.0, 40, 32 + 2, 16, 8, dim_touched=8).to(DEV).train()
    x_gen, feats = seeded((n, 10), 171).to(DEV), seeded((1, n, f), 172).to(DEV)
    grads = []
    for route in ("own", "cat"):
        gen.zero_grad()
        flag = gen(x_gen, adj_dev)
        assert flag.shape == (n, 1) and int((flag != 0).sum()) == 40
        if route == "own":
            loss = model(feats, adj_dev, flag=flag)
        else:
            loss = model(torch.cat((feats[0, :, :-1], flag), dim=1).unsqueeze(0), adj_dev)
        loss.sum().backward()
        grads.append({name: p.grad.cpu().numpy() for name, p in gen.named_parameters()})
    torch.cuda.synchronize()
    assert len(grads[0]) == 12
    for name in grads[0]:
        assert float(np.abs(grads[1][name]).max()) > 0, name
        assert_normwise(grads[0][name], grads[1][name], what=f"Generator {name}.grad through the evaluator")


@pytest.mark.parametrize("tag", ["a_", "b_", "c_"])
def test_the_fixture_on_the_device(tag):
    from pygcn_amd import CSRGraph, GCN_OVER_MLP
    g9 = load_golden("g9_evaluator.npz")
    state, x, _, d = g9_case(g9, tag)
    dims = [int(v) for v in g9["dims"]]
    model = GCN_OVER_MLP(dims[0], dims[1], dims[2], 0.0, dims[5], dims[2] + x.shape[2] - 1 - d, dims[3], dims[4],
                         dim_touched=d)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    graph = CSRGraph(torch.from_numpy(g9["rowptr"]).to(DEV), torch.from_numpy(g9["col"]).to(DEV),
                     torch.from_numpy(g9["val"]).to(DEV), (64, 64))
    xd = x.to(DEV).requires_grad_()
    out = model(xd, graph)
    out.sum().backward()
    torch.cuda.synchronize()
    assert_normwise(out.detach().cpu().numpy(), g9[tag + "out"], what=f"{tag}out")
    assert_normwise(xd.grad[:, :, -1].cpu().numpy(), g9[tag + "dflag"], what=f"{tag}dflag")
    for name, p in model.named_parameters():
        assert_normwise(p.grad.cpu().numpy(), g9[tag + "grad_" + name], what=f"{tag}grad {name}")


def test_no_host_synchronisation_and_the_hip_route():
    """Forward and backward of the model synchronise with the host zero times, with the flag inside x and on its
    own; the sweeps that run are the new ones (no torch.cat of [k, N, ·] size: the pool reads in place)."""
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    model, _ = evaluator(17)
    x, target = model_input(3, n, 17, 181).to(DEV), seeded((3, 1), 183).to(DEV)
    flag = x[:, :, -1].clone().requires_grad_()
    xg = x.clone().requires_grad_()
    F.mse_loss(model(xg, adj_dev), target).backward()          # (first use builds the graph's plans)
    kept = {}

    def forward(**kw):
        kept["loss"] = F.mse_loss(model(kw.pop("x"), adj_dev, **kw), target)

    assert S.count_host_syncs(lambda: forward(x=xg)) == 0
    assert S.count_host_syncs(lambda: kept["loss"].backward()) == 0
    assert S.count_host_syncs(lambda: forward(x=x, flag=flag)) == 0
    assert kept["loss"].grad_fn is not None
    assert S.count_host_syncs(lambda: kept["loss"].backward()) == 0
    assert flag.grad is not None and flag.grad.shape == flag.shape
    from pygcn_amd.models import PoolLayer
    assert S.count_host_syncs(lambda: PoolLayer()(x)) == 0


def test_launches_of_one_step(monkeypatch):
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    model, _ = evaluator(9)
    x = model_input(3, n, 9, 191).to(DEV)
    flag = x[:, :, -1].clone().requires_grad_()
    spy = S.LaunchSpy(monkeypatch)
    model(x, adj_dev, flag=flag).sum().backward()
    torch.cuda.synchronize()
    names = spy.names()
    for name in ("gcn_eval_ingest", "gcn_eval_ingest_backward", "gcn_masked_colsum", "gcn_attn_scores",
                 "gcn_masked_broadcast"):
        assert names.count(name) == 1, (name, names)
    back = [args for name, args in spy.calls if name == "gcn_eval_ingest_backward"][0]
    assert back[2] is None and back[9] is None and back[10] is not None      # no d_wide, no dx: only dflag
    # outside the shape rule (F = 65) the torch composition takes over, with the same contract
    from pygcn_amd.functional import evaluator_ingest
    x65 = seeded((2, 37, 65), 192).to(DEV).requires_grad_()
    before = len(spy.calls)
    wide, mask, esum, nonzero = evaluator_ingest(x65, 8)
    assert len(spy.calls) == before and wide.shape == (37, 16) and esum.shape == (2, 56)
    assert torch.equal(mask, x65[:, :, -1]) and nonzero.tolist() == [37, 37]
