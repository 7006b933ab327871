"""fp64 restatement of the CLIP text tower (`clip.model.CLIP.encode_text` / transformers.CLIPTextModelWithProjection) on a state dict
with the transformers key names: token + position embedding, pre-LN blocks with q scaled by d^-0.5, an additive causal mask and
QuickGELU (x sigmoid(1.702 x)), the final LayerNorm, the row at `eot`, the bias-free projection.  Plain module (not a conftest): the
host tests check it against the fixture and against the library, the GPU tests use it as the reference of the native tower."""
import torch
import torch.nn.functional as F


def attention_ref(q, k, v, scale, dtype=torch.float64):
    """softmax(scale q k^T + causal mask) v on (B, H, S, d) tensors in `dtype`, with torch's own operations."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    S = q.shape[-2]
    mask = torch.full((S, S), float("-inf"), dtype=dtype).triu(1)
    return torch.softmax((q * scale) @ k.transpose(-1, -2) + mask, dim=-1) @ v


def default_eot(ids):
    """encode_text's pooling position: the first position holding the row's largest id."""
    return ids.argmax(dim=1)


def tower_ref(sd, ids, n_head, eot=None, eps=1e-5, dtype=torch.float64):
    """-> (B, P) in `dtype`.  sd: transformers-layout state dict, ids: int64 (B, S)."""
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    B, S = ids.shape
    x = w["text_model.embeddings.token_embedding.weight"][ids] + w["text_model.embeddings.position_embedding.weight"][:S]
    C = x.shape[-1]
    d = C // n_head
    n = 0
    while f"text_model.encoder.layers.{n}.layer_norm1.weight" in w:
        p = f"text_model.encoder.layers.{n}."
        h = F.layer_norm(x, (C,), w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
        q, k, v = (F.linear(h, w[p + f"self_attn.{a}_proj.weight"], w[p + f"self_attn.{a}_proj.bias"])
                   .view(B, S, n_head, d).transpose(1, 2) for a in "qkv")
        a = attention_ref(q, k, v, d ** -0.5, dtype).transpose(1, 2).reshape(B, S, C)
        x = x + F.linear(a, w[p + "self_attn.out_proj.weight"], w[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (C,), w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps)
        h = F.linear(h, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"])
        n += 1
    x = F.layer_norm(x, (C,), w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], eps)
    eot = default_eot(ids) if eot is None else eot
    return F.linear(x[torch.arange(B), eot], w["text_projection.weight"])
