"""Vertex selection — how every policy generator of the fork ends: NN vertices chosen out of N.

  topk_flag(scores, NN)       Generator / Hierarchical_Generator (reference pygcn/models.py:373-377, :398-406):
                                  sorted_indices = torch.argsort(mlp_output, dim=0, descending=True)
                                  topk_mask = torch.where(mlp_output > mlp_output[sorted_indices[NN]], 1/mlp_output, 0)
                                  vac_flag = mlp_output * topk_mask
  sample_without_replacement  SoftGenerator's training step (reference pygcn/rl-policy-generator.py:324-336):
  selection_log_prob              torch.multinomial(attn, NN, replacement=False).tolist()
                                  sum of Categorical(attn).log_prob over the picks

The fork sorts all N scores and, for the draw, walks the picks in a Python loop on the host.  Here the NN
largest of N are found by a radix select (pygcn_amd/csrc/gcn_select.hip), nothing synchronises with the host,
and the draw is an exponential race: the NN largest of p_r / E_r with E_r i.i.d. Exp(1) have the law of NN
draws without replacement with probabilities proportional to p — P(vertex a has the largest key) = p_a / sum p
(the minimum of independent exponentials with rates p_r), and given it, the others' keys are still
independent exponentials by memorylessness: the Plackett-Luce law torch.multinomial(replacement=False) samples.

    kth_largest     gcn_select_kth       [k, n] keys -> the kth largest per window, and how many are greater
    topk_indices    gcn_select_indices   the m vertices above / at that threshold, ascending, ties by low index
    flag_above      gcn_topk_flag        s > thr ? s * (1 / s) : 0
    race_keys       gcn_race_keys        p / Exp(1) from a Philox stream fixed by (seed, window, vertex)

All of them take and return fp32 [k, n] (one row per sample or window) on the HIP device."""
import torch

from . import _native
from .spmm import dropout_seed_for


def _rows(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2
            and t.is_contiguous() and t.shape[0] >= 1 and t.shape[1] >= 1):
        raise RuntimeError(f"{what}: expected a contiguous fp32 [k, n] tensor on the HIP device")
    return t.shape


def kth_largest(keys, kth):
    """(thr fp32 [k], count_gt int32 [k]): per window the `kth`-largest key (1-based) in the selection order
    — -0 is +0, NaN above +inf — and the number of keys strictly greater."""
    k, n = _rows(keys, "kth_largest")
    thr = torch.empty(k, dtype=torch.float32, device=keys.device)
    count_gt = torch.empty(k, dtype=torch.int32, device=keys.device)
    _native.launch("gcn_select_kth", keys.device, keys.data_ptr(), n, k, int(kth), thr.data_ptr(),
                   count_gt.data_ptr(), workspace=_native.lib().gcn_select_workspace_bytes(n, k))
    return thr, count_gt


def topk_indices(keys, m, thr, count_gt):
    """int64 [k, m]: the vertices whose key is above thr[j], then the lowest-index ones equal to it, `m` in all,
    in ascending vertex order; (thr, count_gt) = kth_largest(keys, m)."""
    k, n = _rows(keys, "topk_indices")
    idx = torch.empty((k, int(m)), dtype=torch.int64, device=keys.device)
    _native.launch("gcn_select_indices", keys.device, keys.data_ptr(), n, k, int(m), thr.data_ptr(),
                   count_gt.data_ptr(), idx.data_ptr(), workspace=_native.lib().gcn_select_workspace_bytes(n, k))
    return idx


def flag_above(s, thr, out=None):
    """fp32 [k, n]: s > thr[j] ? s * (1 / s) : 0, each operation rounded once."""
    k, n = _rows(s, "flag_above")
    out = torch.empty_like(s) if out is None else out
    _native.launch("gcn_topk_flag", s.device, s.data_ptr(), n, k, thr.data_ptr(), out.data_ptr())
    return out


def race_keys(p, seed):
    """fp32 [k, n]: p / E with E ~ Exp(1) drawn from Philox4x32-10 at (seed, window, vertex) — the stream
    include/gcn_spmm.h states.  `p` must be finite and >= 0 (not checked: that would read the device).  A
    1-element int64 DEVICE tensor as `seed` is read when the kernel runs (C-ABI gcn_race_keys_dev: a launch
    captured into a hipGraph, spmm.dropout_seed_for); the keys are those of its value as a host seed."""
    k, n = _rows(p, "race_keys")
    keys = torch.empty_like(p)
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != p.device:
            raise RuntimeError("race_keys: a tensor seed must be one int64 on the operand's device")
        _native.launch("gcn_race_keys_dev", p.device, p.data_ptr(), n, k, seed.data_ptr(), keys.data_ptr())
    else:
        _native.launch("gcn_race_keys", p.device, p.data_ptr(), n, k, int(seed) & 0xFFFFFFFFFFFFFFFF, keys.data_ptr())
    return keys


def _vertex_dim(shape):
    """Where the vertices lie: dim 0 of [N] and of the fork's [N, 1]; the last dim of [k, N]."""
    if len(shape) == 1 or (len(shape) == 2 and shape[1] == 1):
        return 0
    if len(shape) == 2:
        return 1
    raise RuntimeError(f"topk_flag: scores {tuple(shape)} are neither [N], [N, 1] nor [k, N]")


def _literal_flag(scores, NN, dim):
    """The reference's lines (pygcn/models.py:373-377), along `dim`."""
    sorted_indices = torch.argsort(scores, dim=dim, descending=True)
    thr = scores.gather(dim, sorted_indices.narrow(dim, NN, 1))
    reverse = torch.reciprocal(scores.detach())
    zero = torch.zeros_like(scores.detach())
    topk_mask = torch.where(scores > thr, reverse, zero)
    return scores * topk_mask


class TopkFlagFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, NN):
        thr, _ = kth_largest(s, NN + 1)
        ctx.save_for_backward(s, thr)
        return flag_above(s, thr)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        # the mask is detached in the reference: d flag / d s = (s > thr ? 1 / s : 0)
        s, thr = ctx.saved_tensors
        mask = torch.where(s > thr.unsqueeze(1), torch.reciprocal(s), torch.zeros_like(s))
        return g * mask, None


def topk_flag(scores, NN):
    """The fork's `vac_flag` (reference pygcn/models.py:373-377): `scores * where(scores > t, 1 / scores, 0)`
    with t the score at index NN of the descending order, i.e. the (NN+1)-th largest; 0 <= NN <= N - 1.  The
    NN largest scores give 1 (a score of 0 gives 0 * inf = NaN, as there), the rest 0; scores EQUAL to t are
    not selected, so ties at the threshold leave fewer than NN ones.  A NaN score sorts above +inf (torch's
    argsort) and is never selected (NaN > t is false).  The mask is detached, as in the fork: the gradient is
    g * (scores > t ? 1 / scores : 0).  One difference on the device: a vertex that is NOT selected gets 0
    whatever its score, where the fork's product `score * 0` leaves NaN for a NaN or infinite score (and -0 for
    a negative one); the selected values are the fork's bits.

    `scores` is [N], the fork's [N, 1] or [k, N] (one row per sample; a 2-D tensor with ONE column is read as
    [N, 1]); the result has its shape and dtype.  fp32 and bf16 (upcast, rounded once at the end) on the HIP
    device run as one autograd node over the radix select and one flag sweep, with no sort and no host
    synchronisation; CPU tensors and other dtypes take the reference's lines."""
    dim = _vertex_dim(scores.shape)
    n = scores.shape[dim]
    NN = int(NN)
    if not 0 <= NN <= n - 1:
        raise RuntimeError(f"topk_flag: needs 0 <= NN <= N - 1, got NN={NN} for N={n}")
    if not (scores.is_cuda and scores.dtype in (torch.float32, torch.bfloat16)):
        return _literal_flag(scores, NN, dim)
    s = scores.to(torch.float32)
    s = (s.reshape(1, n) if dim == 0 else s).contiguous()
    out = TopkFlagFunction.apply(s, NN)
    if dim == 0:
        out = out.reshape(scores.shape)
    return out if out.dtype == scores.dtype else out.to(scores.dtype)


def sample_without_replacement(probs, NN, seed=None):
    """`torch.multinomial(probs, NN, replacement=False)` without the sort, the [N] exponential draw of
    torch's own implementation or a host read: int64 [NN] for probs [N], [k, NN] for [k, N], on probs'
    device, in DRAW ORDER (descending race key, the lower index first on equal keys).  The law is
    torch.multinomial's (module docstring); the stream is this project's, fixed by `seed`.  seed=None draws
    one from the device's generator as a fused dropout launch does (spmm.dropout_seed_for), so
    torch.manual_seed reproduces a run; while the stream is being captured into a hipGraph that is the
    device-resident seed the capture advances, so every replay draws anew.  probs must be finite and >= 0 — NOT checked on the device, where
    torch.multinomial would synchronise to raise; a vertex with probability 0 is picked only when NN exceeds
    the number of positive ones, lowest index first.  CPU tensors go to torch.multinomial."""
    if probs.dim() not in (1, 2):
        raise RuntimeError(f"sample_without_replacement: probs {tuple(probs.shape)} are neither [N] nor [k, N]")
    n, NN = probs.shape[-1], int(NN)
    if not 1 <= NN <= n:
        raise RuntimeError(f"sample_without_replacement: needs 1 <= NN <= N, got NN={NN} for N={n}")
    if not probs.is_cuda:
        return torch.multinomial(probs, NN, replacement=False)
    p = probs.detach().to(torch.float32).reshape(-1, n).contiguous()
    keys = race_keys(p, dropout_seed_for(p) if seed is None else seed)
    idx = topk_indices(keys, NN, *kth_largest(keys, NN))
    # the NN survivors in draw order: a stable descending sort of their keys keeps ascending indices on ties
    order = torch.sort(keys.gather(1, idx), dim=1, descending=True, stable=True).indices
    idx = idx.gather(1, order)
    return idx.view(NN) if probs.dim() == 1 else idx


def selection_log_prob(probs, idx):
    """sum_i log(probs[idx_i]) - NN * log(sum probs): `Categorical(probs).log_prob(idx_i)` summed over the NN
    picks (Categorical normalises its argument) — the fork's `saved_log_probs` entry and
    ReplayBuffer.get_log_prob (reference pygcn/rl-policy-generator.py:335, pygcn/utils.py:516-522).  probs [N]
    with idx [NN] -> a scalar, [k, N] with [k, NN] -> [k]; both sums are taken in double and the result has
    probs' dtype.  Plain torch ops on [NN] and one reduction of [N]: differentiable into whatever made
    `probs` (the attention node), no host synchronisation."""
    picked = probs.gather(-1, idx)
    total = probs.sum(-1, dtype=torch.float64)
    out = torch.log(picked).sum(-1, dtype=torch.float64) - idx.shape[-1] * torch.log(total)
    return out.to(probs.dtype)
