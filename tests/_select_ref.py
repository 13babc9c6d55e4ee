"""Numpy restatement of vertex selection (include/gcn_spmm.h, "Vertex selection"): the total order on fp32, the
k-th largest, the index rule and the race keys with their own Philox4x32-10 — what tests/test_select_cpu.py pins
and tests/test_select_gpu.py holds the HIP kernels against, exactly.  Torch restatements of the fork's Generator
and Hierarchical_Generator (reference pygcn/models.py:358-408) in any dtype give the float64 arbiter for the
fixture g8_generators.npz.  Nothing here imports the native library.

  order_key(x)                 uint32 with the selection order: -0 is +0, NaN above +inf, else numeric
  key_float(t)                 the canonical float of a key (NaN 0x7FC00000, zero +0)
  kth_largest(keys, kth)       (thr fp32 [k], count_gt int32 [k]) of keys [k, n]
  topk_indices(keys, m)        int64 [k, m]: above the m-th largest, then the lowest indices equal to it; ascending
  draw_order(keys, m)          the same m vertices by descending key, lower index first on equal keys
  philox4x32_10(c, key)        counters uint32 [..., 4], key (lo, hi) -> uint32 [..., 4]
  race_keys(p, seed)           fp32 [k, n]: p / E, E = -log((w + 0.5) * 2^-32), w = Philox((r >> 2, window, 1), seed)[r & 3]
  race_statistics(a, b, p)     how far first picks and ordered first-two pairs lie from the Plackett-Luce law, in sigma
  flag(s, thr)                 float32 s > thr ? s * (1 / s) : 0
  assert_flag_exact(...)       a model's vac_flag against the fixture's: the same set, its own s * (1 / s) bitwise
  generator_step(...)          (scores, vac_flag, {name: grad of vac_flag.sum()})
"""
import numpy as np
import torch
import torch.nn.functional as F


def order_key(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    t = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    t[nan] = np.uint32(0xFFFFFFFF)
    return t


def key_float(t):
    t = np.asarray(t, dtype=np.uint32)
    u = np.where((t & np.uint32(0x80000000)) != 0, t & np.uint32(0x7FFFFFFF), ~t).astype(np.uint32)
    u = np.where(t == np.uint32(0xFFFFFFFF), np.uint32(0x7FC00000), u).astype(np.uint32)
    return u.view(np.float32)


def prepared(keys):
    """(order keys, the same sorted along the rows): what kth_largest / topk_indices derive everything from —
    pass it as `pre` to sort a large input once for several ranks."""
    t = order_key(keys)
    return t, np.sort(t, axis=1)


def kth_largest(keys, kth, pre=None):
    t, ts = prepared(keys) if pre is None else pre
    k, n = t.shape
    assert 1 <= kth <= n
    thr = ts[:, n - kth]
    return key_float(thr), (t > thr[:, None]).sum(1).astype(np.int32)


def topk_indices(keys, m, pre=None):
    t, ts = prepared(keys) if pre is None else pre
    k, n = t.shape
    thr = ts[:, n - m]
    out = np.empty((k, m), np.int64)
    for j in range(k):
        gt = np.flatnonzero(t[j] > thr[j])
        eq = np.flatnonzero(t[j] == thr[j])[:m - gt.size]
        out[j] = np.sort(np.concatenate([gt, eq]))
    return out


def draw_order(keys, m):
    t = order_key(keys)
    return np.stack([np.argsort(-t[j].astype(np.int64), kind="stable")[:m] for j in range(t.shape[0])])


def philox4x32_10(counter, key):
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def race_keys(p, seed):
    p = np.asarray(p, dtype=np.float32)
    k, n = p.shape
    r = np.arange(n, dtype=np.int64)
    q = r >> 2
    counter = np.empty((k, n, 4), np.uint64)
    counter[..., 0] = (q & 0xFFFFFFFF)[None, :]
    counter[..., 1] = (q >> 32)[None, :]
    counter[..., 2] = np.arange(k, dtype=np.uint64)[:, None]
    counter[..., 3] = 1
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    word = np.take_along_axis(w, np.broadcast_to((r & 3)[None, :, None], (k, n, 1)), axis=2)[..., 0]
    u = (word.astype(np.float64) + 0.5) * 2.0 ** -32
    with np.errstate(divide="ignore", invalid="ignore"):
        return (p.astype(np.float64) / -np.log(u)).astype(np.float32)


def race_statistics(first, second, p):
    """(max |freq - p| / sigma over the first picks, the same over the ordered first-two pairs against the
    Plackett-Luce value p_a * p_b / (1 - p_a)), sigma = sqrt(q (1 - q) / draws) of each probability q."""
    draws, n = first.size, p.size
    p = p.astype(np.float64) / p.astype(np.float64).sum()
    f1 = np.bincount(first, minlength=n) / draws
    z1 = np.abs(f1 - p) / np.sqrt(p * (1 - p) / draws)
    pair = np.zeros((n, n))
    np.add.at(pair, (first, second), 1.0 / draws)
    q = p[:, None] * p[None, :] / (1 - p[:, None])
    off = ~np.eye(n, dtype=bool)
    assert pair[~off].sum() == 0                          # without replacement
    z2 = np.abs(pair - q)[off] / np.sqrt(q * (1 - q) / draws)[off]
    return float(z1.max()), float(z2.max())


def flag(s, thr):
    """numpy float32 s * (1 / s) under the mask s > thr (thr per row of s [k, n])."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        one = s * (np.float32(1.0) / s)
    return np.where(s > np.asarray(thr, np.float32)[:, None], one, np.float32(0.0)).astype(np.float32)


def assert_flag_exact(got_flag, got_scores, fixture_flag, NN, what=""):
    """What is exact about a vac_flag whose scores agree with the fixture's to rounding only: the CHOSEN SET is
    the fixture's, and every stored value is, bit for bit, the float32 s * (1 / s) of the model's OWN score under
    the mask s > (NN+1)-th largest — a product that is 1 or 1 - 2^-24 depending on the last bits of s, which is
    why the values themselves cannot be held against a run whose scores differ in the last bit."""
    got_flag, got_scores = np.asarray(got_flag, np.float32), np.asarray(got_scores, np.float32)
    fixture_flag = np.asarray(fixture_flag, np.float32)
    assert got_flag.shape == fixture_flag.shape == got_scores.shape, what
    assert np.array_equal(got_flag != 0, fixture_flag != 0), f"{what}: another set of vertices was chosen"
    assert int((got_flag != 0).sum()) == NN, what
    s = got_scores.reshape(1, -1)
    want = flag(s, kth_largest(s, NN + 1)[0]).reshape(got_flag.shape)
    assert np.array_equal(got_flag.view(np.uint32) << 1, want.view(np.uint32) << 1), f"{what}: not s * (1 / s)"  # (+-0 alike)
    for f in (got_flag, fixture_flag):
        assert bool((np.abs(f[f != 0] - 1.0) <= 2.0 ** -24).all()), what


# ------------------------------------------------------------------------ the fork's two generator models
def literal_flag(mlp_output, NN):
    """reference pygcn/models.py:373-377, as written there."""
    sorted_indices = torch.argsort(mlp_output, dim=0, descending=True)
    reverse = torch.reciprocal(mlp_output.detach())
    zero = torch.zeros_like(mlp_output.detach())
    topk_mask = torch.where(mlp_output > mlp_output[sorted_indices[NN]], reverse, zero)
    return mlp_output * topk_mask


def generator_scores(params, x, adj, d, hierarchical):
    h = x[:, :d]
    for i in (1, 2, 3):
        h = F.relu(torch.sparse.mm(adj, h @ params[f"GCNLayer.gc{i}.weight"]) + params[f"GCNLayer.gc{i}.bias"])
    lin = lambda i, t: F.linear(t, params[f"MLPLayers.linear{i}.weight"], params[f"MLPLayers.linear{i}.bias"])  # noqa: E731
    if hierarchical:
        h = torch.cat((h, x[:, d:-1]), dim=1)
        out = lin(3, F.relu(lin(2, F.relu(lin(1, h)))))
        min_value = (torch.ones_like(out) * torch.min(out)).squeeze()
        return torch.where(x[:, -1] == 0, min_value, out.squeeze()).unsqueeze(1)
    h = torch.cat((h, x[:, d:]), dim=1)
    bn = lambda t: F.batch_norm(t, None, None, None, None, True, 0.0, 1e-5)  # noqa: E731
    return lin(3, bn(F.relu(lin(2, bn(F.relu(lin(1, h)))))))


def generator_step(state, x, adj, d, NN, dtype, hierarchical):
    params = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in state.items()}
    scores = generator_scores(params, x.to(dtype), adj.to(dtype), d, hierarchical)
    vac_flag = literal_flag(scores, NN)
    vac_flag.sum().backward()
    return scores.detach().numpy(), vac_flag.detach().numpy(), {k: p.grad.numpy() for k, p in params.items()}


def fixture_case(g8, tag):
    """(state, x, adj sparse CSR float32, dim_touched, NN) of model `tag` ("gen_" / "hier_") of g8_generators.npz."""
    head = tag + "param_"
    state = {name[len(head):]: torch.from_numpy(g8[name]) for name in g8.files if name.startswith(head)}
    n = g8["x"].shape[0]
    adj = torch.sparse_csr_tensor(torch.from_numpy(g8["rowptr"]), torch.from_numpy(g8["col"]).long(),
                                  torch.from_numpy(g8["val"]), (n, n))
    return state, torch.from_numpy(g8["x"]), adj, int(g8["dims"][0]), int(g8["dims"][5])
