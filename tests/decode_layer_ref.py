"""Plain float64 reference of one cached decode step of a post-norm nn.TransformerDecoderLayer (ReLU, eval mode), and the inputs of the
direct p3_decode_layer tests.  Plain torch on the CPU, no project code: tests/test_decode_layer_ref_cpu.py proves the reference against
torch.nn.TransformerDecoderLayer and the probe inputs against the reference; tests/test_decode_layer_gpu.py runs the kernel on the same inputs."""
import math

import torch

D, H, FF, DH = 256, 8, 2048, 32
SCALE = 1.0 / math.sqrt(DH)
MATRICES = ("w_in", "w_so", "w_q", "w_co", "w1", "w2")
VECTORS = ("b_in", "b_so", "b_q", "b_co", "b1", "b2", "g1", "be1", "g2", "be2", "g3", "be3")
PROBE_SCORE = 30.0        # score of a probed key, against a background of order 1
PROBE_VALUE = 2.0         # magnitude of a probed key's value row
CUR_MARGIN = 20.0         # the least lead of the layer's own fresh key where it is the probe


def _layernorm(y, g, b, eps):
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * g + b


def _attend(q, K, V, bias, heads, drop):
    """q [B, D], K / V [B, L, D], bias [B, L] or None -> [B, D]; drop [B] (or None): that key's probability is zeroed and the rest renormalised
    (a negative entry drops nothing)"""
    B, L, Dm = K.shape
    dh = Dm // heads
    s = torch.einsum("bhd,blhd->bhl", q.view(B, heads, dh), K.view(B, L, heads, dh)) / math.sqrt(dh)
    if bias is not None:
        s = s + bias[:, None, :]
    p = torch.softmax(s, -1)
    if drop is not None:
        keep = torch.ones(B, L, dtype=p.dtype)
        for b, j in enumerate(drop.tolist()):
            if j >= 0:
                keep[b, j] = 0.0
        p = p * keep[:, None, :]
        p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhl,blhd->bhd", p, V.view(B, L, heads, dh)).reshape(B, Dm)


def decode_layer_ref(x, kv_self, kv_mem, key_bias, t, w, eps, heads=8, dtype=torch.float64, round_to=None, drop_self=None, drop_mem=None):
    """x [B, D]: the new position's input row; kv_self [B, >= t, 3D]: rows < t are the cached q|k|v rows (rows >= t are never touched);
    kv_mem [B, Lmem, 2D]: the memory's k|v rows; key_bias [B, >= t+1] or None, added to the self-attention scores; w: the layer's tensors
    in p3_decode_layer's naming.  -> dict(qkv [B, 3D], x1, x2, out [B, D]: the three LayerNorm outputs; q_mem: the cross-attention query; a_self, a_mem: the attention outputs).
    round_to: the values the bf16 kernel stores between its stages (q|k|v rows, attention outputs, LayerNorm outputs, hidden layer) are
    rounded to that type and taken back to `dtype`; everything between those points is `dtype` arithmetic."""
    rnd = (lambda v: v.to(round_to).to(dtype)) if round_to is not None else (lambda v: v)
    w = {k: v.to(dtype) for k, v in w.items()}
    x = x.to(dtype)
    B, Dm = x.shape
    qkv = rnd(x @ w["w_in"].T + w["b_in"])
    q, k, v = qkv[:, :Dm], qkv[:, Dm:2 * Dm], qkv[:, 2 * Dm:]
    past = kv_self[:, :t].to(dtype)
    K = torch.cat([past[:, :, Dm:2 * Dm], k[:, None]], 1)
    V = torch.cat([past[:, :, 2 * Dm:], v[:, None]], 1)
    bias = None if key_bias is None else key_bias[:, :t + 1].to(dtype)
    a_self = a = rnd(_attend(q, K, V, bias, heads, drop_self))
    x1 = rnd(_layernorm(a @ w["w_so"].T + w["b_so"] + x, w["g1"], w["be1"], eps))
    q_mem = rnd(x1 @ w["w_q"].T + w["b_q"])
    mem = kv_mem.to(dtype)
    a_mem = a = rnd(_attend(q_mem, mem[..., :Dm], mem[..., Dm:], None, heads, drop_mem))
    x2 = rnd(_layernorm(a @ w["w_co"].T + w["b_co"] + x1, w["g2"], w["be2"], eps))
    hid = rnd(torch.relu(x2 @ w["w1"].T + w["b1"]))
    out = rnd(_layernorm(hid @ w["w2"].T + w["b2"] + x2, w["g3"], w["be3"], eps))
    return dict(qkv=qkv, x1=x1, x2=x2, out=out, q_mem=q_mem, a_self=a_self, a_mem=a_mem)


# ---- inputs of the direct kernel tests ------------------------------------------------------------------------------------------------

def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v) + 1
    return torch.Generator().manual_seed(s % (2 ** 62))


def rounded(v, dt):
    """float64 image of v after it was stored as dt"""
    return v.to(dt).to(torch.float64)


def make_weights(dt, seed=20):
    """one layer of random weights as float64 tensors that dt (matrices) / float32 (vectors) hold exactly: matrices N(0, 1/sqrt(in)), biases
    0.1 N(0, 1), gamma 1 + 0.2 U(-1, 1), beta 0.1 N(0, 1)"""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shapes = dict(w_in=(3 * D, D), w_so=(D, D), w_q=(D, D), w_co=(D, D), w1=(FF, D), w2=(D, FF))
    w = {k: rounded(n(*s) / math.sqrt(s[1]), dt) for k, s in shapes.items()}
    for k, rows in (("b_in", 3 * D), ("b_so", D), ("b_q", D), ("b_co", D), ("b1", FF), ("b2", D), ("be1", D), ("be2", D), ("be3", D)):
        w[k] = rounded(0.1 * n(rows), torch.float32)
    for k in ("g1", "g2", "g3"):
        w[k] = rounded(1.0 + 0.2 * (2.0 * torch.rand(D, generator=g, dtype=torch.float64) - 1.0), torch.float32)
    return w


def make_case(B, t, Lmem, dt, seed):
    """activations and caches 0.5 N(0, 1), one generator per sample: x [B, D], kv_self [B, t, 3D] (the rows in front of the new position),
    kv_mem [B, Lmem, 2D], key_bias [B, t + 1] (zero); float64 values that dt holds exactly"""
    xs, ks, ms = [], [], []
    for b in range(B):
        g = _gen(seed, b)
        xs.append(0.5 * torch.randn(D, generator=g, dtype=torch.float64))
        ks.append(0.5 * torch.randn(t, 3 * D, generator=g, dtype=torch.float64))
        ms.append(0.5 * torch.randn(Lmem, 2 * D, generator=g, dtype=torch.float64))
    return dict(B=B, t=t, Lmem=Lmem, dt=dt, x=rounded(torch.stack(xs), dt), kv_self=rounded(torch.stack(ks), dt), kv_mem=rounded(torch.stack(ms), dt),
                key_bias=torch.zeros(B, t + 1, dtype=torch.float64))


def case_ref(case, w, eps, **kw):
    """the reference of a case: unrounded float64 for fp32 inputs, rounded where the kernel rounds for bf16 inputs"""
    return decode_layer_ref(case["x"], case["kv_self"], case["kv_mem"], case["key_bias"], case["t"], w, eps, heads=H,
                            round_to=torch.bfloat16 if case["dt"] == torch.bfloat16 else None, **kw)


def _probe_key(q):
    """per head the key whose score against q is PROBE_SCORE: 30 q_h / (scale |q_h|^2)"""
    qh = q.view(H, DH)
    return (PROBE_SCORE * qh / (SCALE * (qh * qh).sum(-1, keepdim=True))).reshape(D)


def _probe_value(seed, b):
    return PROBE_VALUE * (2.0 * torch.randint(0, 2, (D,), generator=_gen(seed, b, 7)).to(torch.float64) - 1.0)


MEM_PROBES = {784: (0, 63, 64, 65, 127, 128, 767, 768, 783), 832: (207, 208, 383, 384, 415, 416, 575, 576, 831)}
SELF_PROBES = (0, 63, 64, 95, 96, 207, 208, 383, 384)
SELF_PROBE_T = 384


def mem_probe_case(Lmem, dt, w, eps, seed=300):
    """nine samples, sample b with a one-hot key at memory token MEM_PROBES[Lmem][b] -> (case, jstar)"""
    js = MEM_PROBES[Lmem]
    case = make_case(len(js), 3, Lmem, dt, seed + Lmem)
    q = case_ref(case, w, eps)["q_mem"]                      # the query does not depend on the memory
    for b, j in enumerate(js):
        case["kv_mem"][b, j, :D] = rounded(_probe_key(q[b]), dt)
        case["kv_mem"][b, j, D:] = _probe_value(seed, b)
    return case, torch.tensor(js)


def _own_key_margin(x, w, dt, past_k):
    """least lead over the heads of the fresh key's score over the cached keys' scores, for the input row x"""
    r = lambda v: rounded(v, dt) if dt == torch.bfloat16 else v
    qkv = r(x @ w["w_in"].T + w["b_in"])
    q, k = qkv[:D].view(H, DH), qkv[D:2 * D].view(H, DH)
    own = (q * k).sum(-1) * SCALE
    other = torch.einsum("hd,lhd->hl", q, past_k.view(-1, H, DH)) * SCALE
    return float((own - other.max(-1).values).min())


def self_probe_case(dt, w, eps, seed=400, Lmem=16):
    """nine samples at t = 384, sample b with a one-hot key at position SELF_PROBES[b]; the last probe is the new position itself, whose key
    the layer computes: that sample's input row is searched (direction) and scaled until its own key leads every head by CUR_MARGIN.
    -> (case, jstar)"""
    t = SELF_PROBE_T
    case = make_case(len(SELF_PROBES), t, Lmem, dt, seed)
    bcur = SELF_PROBES.index(t)
    # direction: of many random rows the one whose q_h . k_h (without biases) is positive in every head and largest in its weakest head
    cand = torch.randn(16384, D, generator=_gen(seed, 99), dtype=torch.float64)
    cand = cand / cand.norm(dim=-1, keepdim=True)
    a = ((cand @ w["w_in"][:D].T).view(-1, H, DH) * (cand @ w["w_in"][D:2 * D].T).view(-1, H, DH)).sum(-1).min(-1).values
    best = cand[int(a.argmax())]
    assert float(a.max()) > 0
    for s in range(8, 400, 4):
        x = rounded(best * float(s), dt)
        if _own_key_margin(x, w, dt, case["kv_self"][bcur, :, D:2 * D]) >= CUR_MARGIN + 2.0:
            break
    else:
        raise AssertionError("no input row gives the fresh key a lead of CUR_MARGIN in every head")
    case["x"][bcur] = x
    q = case_ref(case, w, eps)["qkv"][:, :D]                 # the query depends on x alone
    for b, j in enumerate(SELF_PROBES):
        if j < t:
            case["kv_self"][b, j, D:2 * D] = rounded(_probe_key(q[b]), dt)
            case["kv_self"][b, j, 2 * D:] = _probe_value(seed, b)
    return case, torch.tensor(SELF_PROBES)


OUT_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}     # relative Frobenius error of an output row, per sample


def rel_err(got, ref):
    """per-sample relative Frobenius error of [B, D] rows"""
    return (got.to(torch.float64) - ref).norm(dim=-1) / ref.norm(dim=-1)
