"""Test infrastructure: the model under true clip lengths, restated on oracle.wav2vec2's functions.  It
computes what HuggingFace's ``Wav2Vec2ForCTC(input_values, attention_mask, labels)`` computes (tests/test_varlen_host.py pins the
two against each other in float64); dtype follows the state dict.

    compose    perturbed[b][i] = clamp(clean[b][i] + p[..][i], -1, 1) for i < len_b, exactly 0 beyond
    conv stack, feature projection: over all T_e frames of the padded input, unchanged
    zeroing    rows t >= T_b of the feature projection's output are zero before the positional conv (modeling_wav2vec2.py:678-681)
    attention  keys >= T_b of clip b get probability 0 in every layer
    CTC        input_length = T_b per clip, reduction 'sum'
"""
import torch
import torch.nn.functional as F

from oracle import wav2vec2 as OW


def frame_counts(a, lengths):
    """T_b = feat_len(len_b), arch.feat_lengths' formula."""
    return [a.feat_lengths(int(n))[-1] for n in lengths]


def sample_mask(lengths, L, dtype=torch.float64):
    return (torch.arange(L)[None, :] < torch.as_tensor(lengths)[:, None]).to(dtype)


def compose(clean, p, lengths, clamp=True):
    """Attack the utterance, then pad."""
    x = clean + p
    if clamp:
        x = x.clamp(-1, 1)
    return x * sample_mask(lengths, clean.shape[-1], clean.dtype)


def _attention(sd, a, pre, x, key_bias):
    B, T, H = x.shape
    nh, hd = a.num_attention_heads, a.head_dim

    def proj(n):
        return F.linear(x, sd[f"{pre}.{n}.weight"], sd[f"{pre}.{n}.bias"]).view(B, T, nh, hd).transpose(1, 2)

    q, k, v = proj("q_proj"), proj("k_proj"), proj("v_proj")
    p = torch.softmax((q @ k.transpose(-1, -2)) * (hd ** -0.5) + key_bias, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B, T, H)
    return F.linear(o, sd[f"{pre}.out_proj.weight"], sd[f"{pre}.out_proj.bias"])


def _encoder(sd, a, h, frames):
    """oracle.wav2vec2.encoder with the frame mask: zeroed rows, then -inf on the keys >= T_b of every layer."""
    B, T, H = h.shape
    eps, K = a.layer_norm_eps, a.num_conv_pos_embeddings
    valid = torch.arange(T)[None, :] < torch.as_tensor(frames)[:, None]               # (B, T)
    h = h * valid[:, :, None].to(h.dtype)
    key_bias = torch.zeros(B, 1, 1, T, dtype=h.dtype).masked_fill(~valid[:, None, None, :], float("-inf"))
    pc = "wav2vec2.encoder.pos_conv_embed.conv"
    pos = F.conv1d(h.transpose(1, 2), OW.pos_conv_weight(sd), sd[f"{pc}.bias"], padding=K // 2,
                   groups=a.num_conv_pos_embedding_groups)
    if K % 2 == 0:
        pos = pos[:, :, :-1]
    h = h + F.gelu(pos).transpose(1, 2)

    def ln(x, name):
        return F.layer_norm(x, (H,), sd[f"{name}.weight"], sd[f"{name}.bias"], eps=eps)

    def ffn(x, pre):
        y = F.gelu(F.linear(x, sd[f"{pre}.intermediate_dense.weight"], sd[f"{pre}.intermediate_dense.bias"]))
        return F.linear(y, sd[f"{pre}.output_dense.weight"], sd[f"{pre}.output_dense.bias"])

    if not a.do_stable_layer_norm:
        h = ln(h, "wav2vec2.encoder.layer_norm")
    for l in range(a.num_hidden_layers):
        pre = f"wav2vec2.encoder.layers.{l}"
        if a.do_stable_layer_norm:
            h = h + _attention(sd, a, f"{pre}.attention", ln(h, f"{pre}.layer_norm"), key_bias)
            h = h + ffn(ln(h, f"{pre}.final_layer_norm"), f"{pre}.feed_forward")
        else:
            h = ln(h + _attention(sd, a, f"{pre}.attention", h, key_bias), f"{pre}.layer_norm")
            h = ln(h + ffn(h, f"{pre}.feed_forward"), f"{pre}.final_layer_norm")
    if a.do_stable_layer_norm:
        h = ln(h, "wav2vec2.encoder.layer_norm")
    return h


def logits_of(sd, a, x, lengths):
    """(B, L) composed waveform (zero beyond len_b) -> (B, T_e, V) logits; rows >= T_b are whatever the pad rows give."""
    f = OW.feature_encoder(sd, a, x).transpose(1, 2)
    C = f.shape[-1]
    f = F.layer_norm(f, (C,), sd["wav2vec2.feature_projection.layer_norm.weight"],
                     sd["wav2vec2.feature_projection.layer_norm.bias"], eps=a.layer_norm_eps)
    h = F.linear(f, sd["wav2vec2.feature_projection.projection.weight"], sd["wav2vec2.feature_projection.projection.bias"])
    h = _encoder(sd, a, h, frame_counts(a, lengths))
    return F.linear(h, sd["lm_head.weight"], sd["lm_head.bias"])


def ctc_loss_of(a, logits, labels, lengths, reduction="sum"):
    """modeling_wav2vec2.py's CTC branch with input_lengths = T_b (log_softmax in float32, as HF computes it)."""
    mask = labels >= 0
    lp = F.log_softmax(logits, dim=-1, dtype=torch.float32).transpose(0, 1)
    return F.ctc_loss(lp, labels.masked_select(mask), torch.tensor(frame_counts(a, lengths), dtype=torch.long), mask.sum(-1),
                      blank=a.pad_token_id, reduction=reduction, zero_infinity=False)


def forward(sd, a, x, labels, lengths):
    logits = logits_of(sd, a, x, lengths)
    return ctc_loss_of(a, logits, labels, lengths), logits


def step_reference(sd, a, clean, p, labels, lengths, rows=False, direction=1.0):
    """loss, logits and the gradient of direction * loss wrt p under lengths: p (L,) / (1, L) universal (rows=False) or (B, L) per clip;
    the gradient has the shape of p."""
    pr = p.clone().requires_grad_(True)
    x = compose(clean, pr if rows else pr.reshape(1, -1), lengths)
    loss, logits = forward(sd, a, x, labels, lengths)
    (direction * loss).backward()
    return float(loss.detach()), logits.detach(), pr.grad.detach()
