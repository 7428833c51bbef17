"""Float64 restatement of the training forward's loss (ParlerTTSForCausalLM.forward with labels): which positions count, the per-token negative
log-likelihood, the per-codebook reductions and their weighting. Takes logits; knows nothing of how they were made."""
import math

import torch


def counted_mask(input_ids, labels, bos_token_id, eos_token_id, vocab_size=None):
    """input_ids int64 [B*K, T] (or [B, K, T]), labels int64 [B, T, K] -> bool [B, T, K]: the label is neither -100 nor BOS and the input column is
    not EOS. With ``vocab_size``: a label outside [0, V) never counts (the engine's rule; torch's CrossEntropyLoss refuses such a target)."""
    B, T, K = labels.shape
    inp = input_ids.reshape(B, K, T).transpose(1, 2)
    m = (labels != -100) & (labels != bos_token_id) & (inp != eos_token_id)
    if vocab_size is not None:
        m = m & (labels >= 0) & (labels < vocab_size)
    return m


def token_nll(logits, labels, counted):
    """logits [B*K, Q, V] (the last T positions are the labelled ones), labels [B, T, K], counted bool [B, T, K] -> float64 [B, T, K]:
    logsumexp - logit[label] where counted, 0 elsewhere. Also returns (lse, picked) for error bounds."""
    B, T, K = labels.shape
    lg = logits.to(torch.float64).reshape(B, K, -1, logits.shape[-1])[:, :, -T:].transpose(1, 2)  # [B, T, K, V]
    lse = torch.logsumexp(lg, dim=-1)
    picked = torch.gather(lg, -1, labels.clamp(0, lg.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
    z = torch.zeros_like(lse)
    return torch.where(counted, lse - picked, z), torch.where(counted, lse, z), torch.where(counted, picked, z)


def reduce_loss(nll, counted, loss_reduction="mean", codebook_weights=None):
    """nll [B, T, K], counted [B, T, K] -> (loss, per_codebook_losses [K]) in float64. Per codebook: the mean (nan without a counted position, as
    torch gives) or the sum (0 then) over the counted positions; then sum_k w_k loss_k / sum_k w_k, or sum_k loss_k / K without weights."""
    if loss_reduction not in ("mean", "sum"):
        raise ValueError(loss_reduction)
    K = nll.shape[-1]
    c = counted.to(torch.float64)
    s = (nll.to(torch.float64) * c).sum(dim=(0, 1))
    per = s / c.sum(dim=(0, 1)) if loss_reduction == "mean" else s
    if codebook_weights is not None:
        w = torch.tensor(list(codebook_weights), dtype=torch.float64)
        loss = (per * w).sum() / w.sum()
    else:
        loss = per.sum() / K
    return loss, per


def loss_from_logits(logits, input_ids, labels, bos_token_id, eos_token_id, loss_reduction="mean", codebook_weights=None):
    cm = counted_mask(input_ids, labels, bos_token_id, eos_token_id)
    nll, _, _ = token_nll(logits, labels, cm)
    return reduce_loss(nll, cm, loss_reduction, codebook_weights)


def kernel_bound(lse, picked, vocab_size):
    """Analytic bound of the fused kernel's nll against the float64 cross-entropy of ITS OWN fp32 logits, per position:
      V * 2^-24            the fp32 sum of V terms in (0, 1] (relative error of the sum <= V * 2^-24 -> absolute error of its logarithm)
      8 ulp32(|lse|)       base-2 scaling of the logits, exp2 / log2 instructions (<= 1 ulp each on their results), the multiplication by ln 2
      4 ulp32(|picked|)    the final subtraction rounds at the larger magnitude
    with ulp32(x) <= 2^-23 * max(|x|, 1)."""
    u = 2.0 ** -23
    return vocab_size * 2.0 ** -24 + 8 * u * lse.abs().clamp(min=1.0) + 4 * u * picked.abs().clamp(min=1.0)


def isclose_nan(a, b, tol):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol
