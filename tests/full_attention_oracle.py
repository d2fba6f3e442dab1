"""fp64 restatement of LoFTREncoderLayer / LocalFeatureTransformer with FullAttention (transformer.py:32-40, :65-94, :133-171;
linear_attention.py:64-95), written from the math: per head (D = d_model / nhead) A = softmax(Q K^T / sqrt(D)) over the source
tokens, message = A V; no feature map, no V / S, no dropout (use_dropout = False upstream); the merge / norm1 / MLP / norm2 /
residual tail as in the linear layer.  Unmasked only (a masked forward with a cross layer raises upstream).  Test infrastructure."""
import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def full_attention(q, k, v):
    """q [B, L, H, D], k / v [B, S, H, D] -> [B, L, H, D]"""
    logits = torch.einsum("nlhd,nshd->nlsh", q, k) / q.size(3) ** 0.5
    return torch.einsum("nlsh,nshd->nlhd", torch.softmax(logits, dim=2), v)


def encoder_layer(sd, p, nhead, x, source):
    B, _, C = x.shape
    D = C // nhead
    w = lambda n: sd[p + "." + n].to(x.dtype)
    q = F.linear(x, w("q_proj.weight")).view(B, -1, nhead, D)
    k = F.linear(source, w("k_proj.weight")).view(B, -1, nhead, D)
    v = F.linear(source, w("v_proj.weight")).view(B, -1, nhead, D)
    msg = F.linear(full_attention(q, k, v).reshape(B, -1, C), w("merge.weight"))
    msg = F.layer_norm(msg, (C,), w("norm1.weight"), w("norm1.bias"), LN_EPS)
    msg = F.linear(F.relu(F.linear(torch.cat([x, msg], dim=2), w("mlp.0.weight"))), w("mlp.2.weight"))
    msg = F.layer_norm(msg, (C,), w("norm2.weight"), w("norm2.bias"), LN_EPS)
    return x + msg


def local_feature_transformer(sd, name, tcfg, feat3d_cn, feat2d):
    """feat3d_cn [B, C, N] (transposed first, transformer.py:145), feat2d [B, L, C] -> (f3, f2), fp64.  Cross layers update both
    streams from the pre-update tensors; final_proj is never applied (as the linear restatement in oracle/onepose_oracle.py)."""
    f3 = feat3d_cn.transpose(1, 2).double()
    f2 = feat2d.double()
    for i, kind in enumerate(list(tcfg["layer_names"]) * tcfg["layer_iter_n"]):
        p = "%s.layers.%d" % (name, i)
        if kind == "self":
            f2, f3 = encoder_layer(sd, p, tcfg["nhead"], f2, f2), encoder_layer(sd, p, tcfg["nhead"], f3, f3)
        elif kind == "cross":
            f2, f3 = encoder_layer(sd, p, tcfg["nhead"], f2, f3), encoder_layer(sd, p, tcfg["nhead"], f3, f2)
        else:
            raise NotImplementedError(kind)
    return f3, f2
