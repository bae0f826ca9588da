"""p3_decode_layer (one launch per decoder layer and decode step) against the 11-launch chain it replaces (Decoder._decode_step, the body
of the reference's Decoder.predict loop, model_pix2poly.py:187-219), in bf16 and (r03) in the fp32 parity mode."""
import pytest
import torch

from oracle import p3_oracle as O
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _decoder(seed, layers=2, cd=torch.bfloat16):
    from pixelspointspolygons_amd.pix2poly import Decoder
    sd = O.make_state_dict("image", dict(dim=64, depth=2, heads=2, mlp=128, patch=8, img=32, eps=1e-6), seed=seed, n_vertices=10,
                           dec_dim=256, dec_layers=layers)
    dec = Decoder(vocab_size=O.VOCAB, encoder_len=16, dim=256, num_heads=8, num_layers=layers, max_len=2 * 10 + 2, pad_idx=O.PAD)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    dec.cd = cd
    return dec.to(DEV).eval(), O


@pytest.mark.parametrize("B", [1, 3, 9])
def test_fused_layer_matches_the_launch_chain(B, monkeypatch):
    dec, O = _decoder(77)
    enc = (torch.randn(B, 16, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(DEV)
    outs = {}
    with torch.no_grad():
        for name, fused, cluster in (("chain", False, "4"), ("fused4", True, "4"), ("fused1", True, "1")):
            dec.fused_decode = fused
            monkeypatch.setenv("P3_DECODE_CLUSTER", cluster)
            dec._decode_state = None
            toks, feats = dec.generate_cached(enc, 21, O.BOS)
            outs[name] = (toks.clone(), feats.float().clone())
            toks2, feats2 = dec.generate_cached(enc, 21, O.BOS)
            assert torch.equal(toks, toks2) and torch.equal(feats, feats2), name            # deterministic (partials summed in member order)
    ref_t, ref_f = outs["chain"]
    for name in ("fused4", "fused1"):
        t, f = outs[name]
        # same roundings at the same places, different summation order inside the dot products: bf16-level agreement on the features
        err = float((f - ref_f).norm() / ref_f.norm())
        assert err < 2e-2, (name, err)
        same = (t == ref_t).float().mean().item()
        assert same == 1.0 or err < 5e-3, (name, same, err)


@pytest.mark.parametrize("B", [1, 5])
def test_fused_fp32_layer_matches_the_fp32_launch_chain(B, monkeypatch):
    """fp32 (parity mode): nothing is rounded between the stages; the fused layer's dot products are summed in another order than the MFMA
    GEMMs of the chain, so features agree to fp32 rounding (2e-5 after 21 steps x 2 layers), tokens are identical, both cluster forms."""
    dec, O = _decoder(77, cd=torch.float32)
    enc = (torch.randn(B, 16, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(DEV)
    outs = {}
    with torch.no_grad():
        for name, fused, cluster in (("chain", False, "4"), ("fused4", True, "4"), ("fused1", True, "1")):
            dec.fused_decode = fused
            monkeypatch.setenv("P3_DECODE_CLUSTER", cluster)
            dec._decode_state = None
            toks, feats = dec.generate_cached(enc, 21, O.BOS)
            outs[name] = (toks.clone(), feats.float().clone())
            toks2, feats2 = dec.generate_cached(enc, 21, O.BOS)
            assert torch.equal(toks, toks2) and torch.equal(feats, feats2), name
    ref_t, ref_f = outs["chain"]
    for name in ("fused4", "fused1"):
        t, f = outs[name]
        assert torch.equal(t, ref_t), name
        assert float((f - ref_f).norm() / ref_f.norm()) < 2e-5, (name, float((f - ref_f).norm() / ref_f.norm()))


def test_fused_fp32_decode_reproduces_the_reference_golden_tokens():
    d, _ = load_golden("greedy_d256.npz")
    dec, O = _decoder(77, cd=torch.float32)
    with torch.no_grad():
        toks, _ = dec.generate_cached(d["enc"].to(DEV), 21, O.BOS)
    assert dec._fused_step_ok() and torch.equal(toks.cpu(), d["tokens"])


def test_fused_decode_reproduces_the_reference_golden_tokens():
    """greedy_d256.npz holds the reference decoder's own greedy sequence (fp32); the bf16 fused path must pick the same tokens."""
    d, _ = load_golden("greedy_d256.npz")
    dec, O = _decoder(77)
    enc = d["enc"].to(DEV)
    with torch.no_grad():
        dec.fused_decode = True
        toks, _ = dec.generate_cached(enc, 21, O.BOS)
        dec.fused_decode = False
        dec._decode_state = None
        toks_chain, _ = dec.generate_cached(enc, 21, O.BOS)
    assert torch.equal(toks, toks_chain)
    if torch.equal(toks_chain.cpu(), d["tokens"]):          # bf16 rounding may legitimately move a near-tie of the fp32 golden
        assert torch.equal(toks.cpu(), d["tokens"])


def test_cluster_barrier_never_gave_up_and_graph_replay_is_identical():
    dec, O = _decoder(5, layers=3)
    enc = (torch.randn(8, 16, 256, generator=torch.Generator().manual_seed(1)) * 0.5).to(DEV)
    with torch.no_grad():
        want = dec.generate_cached(enc, 21, O.BOS)
        want = (want[0].clone(), want[1].clone())
        for _ in range(3):                               # call 1 eager, call 2 captures, call 3 replays
            got = dec.generate_cached(enc, 21, O.BOS, graphs=True)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    st = dec._decode_state
    assert st["dl_scratch"] is not None and int(st["dl_scratch"][2]) == 0            # no barrier hit its spin limit
    assert int(st["dl_scratch"][1][:, 0].abs().sum()) == 0                          # arrival counters are back at zero


def test_a_given_up_cluster_barrier_is_detected_and_the_decode_redone_without_clusters():
    """when a cluster member's spin limit is hit the kernel raises the error flag and its sums are invalid.
    generate_cached reads the flag once per call; on error it resets the barrier words and redoes the decode with one workgroup per
    sample (no co-residency needed).  Simulated by raising the flag by hand after a normal run: the tokens must equal the cluster = 1 path."""
    dec, O = _decoder(5, layers=2)
    enc = (torch.randn(4, 16, 256, generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV)
    with torch.no_grad():
        want_t, want_f = (t.clone() for t in dec.generate_cached(enc, 21, O.BOS, graphs=True))     # eager pass, state kept
        st = dec._decode_state
        assert st["dl_scratch"] is not None
        st["dl_scratch"][2].fill_(1)                         # as if a barrier had given up
        st["dl_scratch"][1][0, 0] = 3                        # ... leaving an arrival counter behind
        got_t, got_f = dec.generate_cached(enc, 21, O.BOS, graphs=True)
        st = dec._decode_state
        assert st.get("dl_cluster_failed") and st["dl_scratch"] is None
        assert torch.equal(got_t, want_t)
        assert float((got_f.float() - want_f.float()).norm() / want_f.float().norm()) < 2e-2       # cluster = 1 sums in another order
        again_t, _ = dec.generate_cached(enc, 21, O.BOS, graphs=True)                               # and stays on the safe path
        assert torch.equal(again_t, want_t)


def test_coresident_bound_comes_from_the_device():
    from pixelspointspolygons_amd import hip
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert hip.coresident_workgroups(torch.device("cuda:0"), 2) == 2 * n and n >= 1


def test_decode_layer_rejects_what_it_was_not_built_for():
    from pixelspointspolygons_amd import hip
    x = torch.zeros(2, 128, dtype=torch.bfloat16, device=DEV)
    w = {k: torch.zeros(4, 4, dtype=torch.bfloat16, device=DEV) for k in ("w_in", "w_so", "w_q", "w_co", "w1", "w2")}
    w.update({k: torch.zeros(4, device=DEV) for k in ("b_in", "b_so", "b_q", "b_co", "b1", "b2", "g1", "be1", "g2", "be2", "g3", "be3")})
    with pytest.raises(hip.P3Error):
        hip.decode_layer(x, x.clone(), torch.zeros(2, 4, 384, dtype=torch.bfloat16, device=DEV), torch.zeros(2, 4, 256, dtype=torch.bfloat16, device=DEV),
                         None, 0, 8, w, 1e-5)


# ---- direct tests of hip.decode_layer: one launch on prepared caches against the float64 reference of tests/decode_layer_ref.py, at the shapes
# where the pass / batch structure of the four instantiations changes (attend_reg: 13 passes of 64 keys; attend<4, float>: batches of 6 x 64;
# attend<1, bf16>: 13 x 16; attend<1, float>: 6 x 16).  Inputs sit in NaN-poisoned buffers, the output in a guarded view (tests/guard.py).
from tests import decode_layer_ref as R
from tests import guard as G

EPS = 1e-5
BF, F32 = torch.bfloat16, torch.float32
INSTANCES = [pytest.param(c, dt, id=f"c{c}-{'bf16' if dt == BF else 'fp32'}") for c in (4, 1) for dt in (BF, F32)]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    yield
    _cache.clear()


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _weights(dt, seed=20):
    """(float64 reference tensors, device tensors: matrices in dt, vectors fp32) of one layer; built once per dtype and never changed"""
    def make():
        w = R.make_weights(dt, seed)
        return w, {k: v.to(dt if k in R.MATRICES else F32).to(DEV).contiguous() for k, v in w.items()}
    return _memo(("w", dt, seed), make)


def _bits(t):
    return t.view(G._INT[t.element_size()])


def _poison(n, dt):
    es = torch.empty((), dtype=dt).element_size()
    return torch.full((n,), G.POISON[es], dtype=G._INT[es], device=DEV).view(dt)


def _x_out(B, ld, dt):
    """a guarded [B, 256] output of row stride ld (steps * 256: what feats[:, t] has in decode), shared by the tests of one shape: every launch
    starts from a view full of the sentinel"""
    view, guard = _memo(("x_out", B, ld, dt), lambda: G.guarded(B, R.D, dt, ld=ld, device=DEV))
    _bits(view).fill_(G.SENTINEL[view.element_size()])
    return view, guard


def _cluster_or_skip(cluster, B):
    from pixelspointspolygons_amd import hip
    if cluster == 4:
        if hip.coresident_workgroups(torch.device("cuda:0"), 2) < 72:
            pytest.skip("partition smaller than 72 co-resident workgroups")
        return hip.decode_layer_scratch(B, torch.device("cuda:0"))
    return None


class _Placed:
    """the tensors of a case on the device, placed so that a stray read returns NaN and a stray write is seen"""

    def __init__(self, case, steps, x_out=None):
        B, t, Lmem, dt = case["B"], case["t"], case["Lmem"], case["dt"]
        assert steps > t
        D = R.D
        self.case, self.steps = case, steps
        self.kv_self = _poison(B * steps * 3 * D, dt).view(B, steps, 3 * D)          # rows >= t: poison
        self.kv_self[:, :t] = case["kv_self"].to(dt)
        self.mem_buf = _poison((B * Lmem + 64) * 2 * D, dt)                            # NaN rows follow the last sample
        self.kv_mem = self.mem_buf[:B * Lmem * 2 * D].view(B, Lmem, 2 * D)
        self.kv_mem.copy_(case["kv_mem"].to(dt))
        self.x_in = G.poisoned(case["x"].to(dt), extra_rows=2, front_rows=2, device=DEV)
        self.kb_buf = _poison(B * (steps + 8), F32).view(B, steps + 8)
        self.key_bias = self.kb_buf[:, :steps + 3]                                     # row stride steps + 8; entries > t: NaN
        self.key_bias[:, :t + 1] = case["key_bias"].to(F32)
        self.x_out, self.guard = _x_out(B, steps * D, dt) if x_out is None else x_out


def _launch(p, w, scratch):
    """one launch + every check that needs no reference -> (x_out [B, D], cache row t [B, 3D]) as float64 on the CPU"""
    from pixelspointspolygons_amd import hip
    case, t = p.case, p.case["t"]
    ro = {"kv_mem": p.mem_buf, "x_in": p.x_in, "key_bias": p.kb_buf, **w}
    before = {k: _bits(v).clone() for k, v in ro.items()}
    kv_before = _bits(p.kv_self).clone()
    gen_before = scratch[1][:, 1].clone() if scratch is not None else None
    hip.decode_layer(p.x_in, p.x_out, p.kv_self, p.kv_mem, p.key_bias, t, R.H, w, EPS, scratch=scratch)
    torch.cuda.synchronize()
    if scratch is not None:
        assert int(scratch[2].item()) == 0, "a cluster barrier gave up"
        assert int(scratch[1][:, 0].abs().sum()) == 0, "arrival counters not back at zero"
        assert torch.equal(scratch[1][:, 1] - gen_before, torch.full_like(gen_before, 3)), "three barriers per launch and sample"
    assert not torch.isnan(p.x_out).any(), "NaN in x_out: something at or beyond Lk was read"
    kv_now = _bits(p.kv_self)
    other = torch.ones(p.steps, dtype=torch.bool, device=DEV)
    other[t] = False
    assert torch.equal(kv_now[:, other], kv_before[:, other]), "a kv_self row other than t changed"
    assert not torch.isnan(p.kv_self[:, t]).any(), "poison left in (or NaN written to) row t of kv_self"
    for k, v in ro.items():
        assert torch.equal(_bits(v), before[k]), f"read-only input {k} changed"
    try:
        p.guard.check()
    except AssertionError:
        p.guard.rearm()                      # the guarded buffer is shared: the next test starts from what it holds now
        raise
    return p.x_out.double().cpu(), p.kv_self[:, t].double().cpu()


class _NoGuard:
    def check(self):
        pass

    rearm = check


_worst = {}


def _compare(group, name, case, wref, out, row, ref=None):
    """cache row t against the derived bound of a 256-term fp32 dot product (bf16: + one rounding), x_out per sample against the reference"""
    dt = case["dt"]
    ref = R.case_ref(case, wref, EPS) if ref is None else ref
    raw = case["x"] @ wref["w_in"].T + wref["b_in"]
    bound = 256 * 2.0 ** -24 * (case["x"].abs() @ wref["w_in"].abs().T + wref["b_in"].abs())
    if dt == BF:
        bound = bound + 2.0 ** -8 * raw.abs()
        assert torch.equal(ref["qkv"], R.rounded(raw, BF))
    else:
        assert torch.equal(ref["qkv"], raw)
    row_ratio = float(((row - raw).abs() / bound).max())
    err = float(R.rel_err(out, ref["out"]).max())
    k = (group, "bf16" if dt == BF else "fp32")
    _worst[k] = (max(_worst.get(k, (0, 0))[0], row_ratio), max(_worst.get(k, (0, 0))[1], err))
    print(f"[decode_layer_direct] {group} {name}: cache row worst |err| / bound {row_ratio:.3e}, x_out worst rel err {err:.3e} (tol {R.OUT_TOL[dt]:.0e}); "
          f"group so far {_worst[k][0]:.3e} {_worst[k][1]:.3e}")
    assert row_ratio <= 1.0, (name, row_ratio)
    assert err < R.OUT_TOL[dt], (name, err)
    return ref


def _run(group, name, case, cluster, steps, ref=None):
    wref, w = _weights(case["dt"])
    out, row = _launch(_Placed(case, steps), w, _cluster_or_skip(cluster, case["B"]))
    _compare(group, f"c{cluster} {name}", case, wref, out, row, ref)
    return out


def _ref_of(key, case_fn, dt):
    """(case, reference) computed once and shared by the cluster forms"""
    def make():
        case = case_fn()
        return case, R.case_ref(case, _weights(dt)[0], EPS)
    return _memo(("case",) + key + (dt,), make)


# 1. memory-length edges: the pass and batch edges of all four attention routines (16 / 64 keys per pass; 96 / 208 / 384 / 832 per batch) + 784
MEM_EDGES = [1, 15, 16, 17, 63, 64, 65, 96, 97, 208, 209, 384, 385, 416, 417, 768, 769, 784, 831, 832]


@pytest.mark.parametrize("Lmem", MEM_EDGES)
@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_memory_length_edges(cluster, dt, Lmem):
    case, ref = _ref_of(("mem", Lmem), lambda: R.make_case(9, 3, Lmem, dt, seed=1000 + Lmem), dt)
    _run("1 memory length", f"Lmem {Lmem}", case, cluster, 8, ref)


@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_sequences_beyond_832_are_refused_and_nothing_is_written(cluster, dt):
    from pixelspointspolygons_amd import hip
    _, w = _weights(dt)
    for Lmem, steps in ((833, 8), (16, 833)):
        p = _Placed(R.make_case(9, 3, Lmem, dt, seed=7), steps, x_out=_x_out(9, 8 * R.D, dt))
        kv_before = _bits(p.kv_self).clone()
        with pytest.raises(hip.P3Error):
            hip.decode_layer(p.x_in, p.x_out, p.kv_self, p.kv_mem, p.key_bias, 3, R.H, w, EPS, scratch=_cluster_or_skip(cluster, 9))
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.kv_self), kv_before)
        p.guard.check(valid=torch.zeros(9, R.D, dtype=torch.bool))              # the view still holds the sentinel, the bands too


# 2. position edges: cur at the first and last slot of a pass and of a load batch
POS_EDGES = [0, 1, 15, 16, 63, 64, 65, 95, 96, 127, 128, 207, 208, 383, 384, 385]


@pytest.mark.parametrize("t", POS_EDGES)
@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_position_edges(cluster, dt, t):
    case, ref = _ref_of(("pos", t), lambda: R.make_case(9, t, 16, dt, seed=2000 + t), dt)
    _run("2 position", f"t {t}", case, cluster, 390, ref)


@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_last_position_of_the_longest_cache(cluster, dt):
    case, ref = _ref_of(("pos", 831), lambda: R.make_case(9, 831, 16, dt, seed=2831), dt)
    _run("2 position", "t 831 of 832", case, cluster, 832, ref)


# 3. one-hot key probes: one key per sample takes the whole softmax, so a lost, doubled or misplaced key is an error of order 1
#    (tests/test_decode_layer_ref_cpu.py proves that from the reference alone)
@pytest.mark.parametrize("Lmem", [784, 832])
@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_one_hot_memory_key(cluster, dt, Lmem):
    case, ref = _ref_of(("probe_mem", Lmem), lambda: R.mem_probe_case(Lmem, dt, _weights(dt)[0], EPS)[0], dt)
    _run("3 probes", f"memory probes of Lmem {Lmem}", case, cluster, 8, ref)


@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_one_hot_position_key(cluster, dt):
    case, ref = _ref_of(("probe_self",), lambda: R.self_probe_case(dt, _weights(dt)[0], EPS)[0], dt)
    _run("3 probes", "position probes at t 384", case, cluster, 390, ref)


# 4. key_bias
def _bias_case(kind, dt):
    t = 200
    case = R.make_case(9, t, 16, dt, seed=4000)
    g = torch.Generator().manual_seed(4001)
    if kind == "third":                       # the decoder's own usage: +1.0 at a random third of the positions, another third per sample
        case["key_bias"] = (torch.rand(9, t + 1, generator=g) < 1 / 3).double()
        assert len({tuple(r.tolist()) for r in case["key_bias"]}) == 9
    else:
        case["key_bias"] = torch.full((9, t + 1), -30.0, dtype=torch.float64)
        case["key_bias"][:, [0, 64, 200]] = 0.0
    return case


@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_key_bias_per_sample(cluster, dt):
    case, ref = _ref_of(("bias", "third"), lambda: _bias_case("third", dt), dt)
    _run("4 key_bias", "+1 on a third", case, cluster, 390, ref)


@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_key_bias_suppression_equals_the_three_key_cache(cluster, dt):
    case, ref = _ref_of(("bias", "suppress"), lambda: _bias_case("suppress", dt), dt)
    out = _run("4 key_bias", "-30 on all but {0, 64, 200}", case, cluster, 390, ref)
    small = dict(case, t=2, kv_self=case["kv_self"][:, [0, 64]].clone(), key_bias=torch.zeros(9, 3, dtype=torch.float64))
    out3 = _run("4 key_bias", "the three keys alone, t 2", small, cluster, 8)
    err = float(R.rel_err(out3, out).max())
    print(f"[decode_layer_direct] 4 key_bias c{cluster}: suppressed against three-key launch {err:.3e}")
    assert err < R.OUT_TOL[dt], err


# 5. the dense production shape: both cluster forms meet the bound, and a repeated launch is bit-identical
@pytest.mark.parametrize("B", [1, 8, 9])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_direct_cluster_forms_agree_at_the_production_shape(dt, B):
    case, ref = _ref_of(("dense", B), lambda: R.make_case(B, 384, 784, dt, seed=5000 + B), dt)
    for cluster in (1, 4):
        first = _run("5 production shape", f"B {B}", case, cluster, 390, ref)
        again = _run("5 production shape", f"B {B} again", case, cluster, 390, ref)
        assert torch.equal(first, again), cluster


# 6. two layers chained (xa -> xb as Decoder._decode_step does) over three consecutive positions, one exchange / sync scratch for all six launches
@pytest.mark.parametrize("cluster,dt", INSTANCES)
def test_direct_two_layers_chained_over_three_positions(cluster, dt):
    B, D, steps, Lmem = 9, R.D, 72, 16
    layers = [_weights(dt, 20), _weights(dt, 21)]
    scratch = _cluster_or_skip(cluster, B)
    base = R.make_case(B, 63, Lmem, dt, seed=6000)
    mems = [base["kv_mem"], R.make_case(B, 0, Lmem, dt, seed=6001)["kv_mem"]]
    caches = [base["kv_self"], R.make_case(B, 63, Lmem, dt, seed=6002)["kv_self"]]                  # the reference's caches, grown by its own rows
    placed = [_Placed(dict(base, kv_self=caches[li], kv_mem=mems[li]), steps) for li in range(2)]
    xa = torch.empty(B, D, dtype=dt, device=DEV)
    for t in (63, 64, 65):
        x = R.make_case(B, 0, 1, dt, seed=6100 + t)["x"]
        x_dev = G.poisoned(x.to(dt), device=DEV)
        kb = torch.zeros(B, t + 1, dtype=torch.float64)
        cur = x
        for li in range(2):
            case = dict(B=B, t=t, Lmem=Lmem, dt=dt, x=cur, kv_self=caches[li], kv_mem=mems[li], key_bias=kb)
            ref = R.case_ref(case, layers[li][0], EPS)
            caches[li] = torch.cat([caches[li], ref["qkv"][:, None]], 1)
            cur = ref["out"]
        # the kernel's caches keep the rows the kernel wrote; only position, input and bias change between the steps
        outs = []
        for li in range(2):
            p = placed[li]
            p.case = dict(p.case, t=t)
            p.key_bias[:, :t + 1] = 0.0
            p.x_in = x_dev if li == 0 else xa
            if li == 0:
                keep = (p.x_out, p.guard)
                p.x_out, p.guard = xa, _NoGuard()
            out, row = _launch(p, layers[li][1], scratch)
            if li == 0:
                p.x_out, p.guard = keep
            outs.append(out)
        err = float(R.rel_err(outs[1], cur).max())
        k = ("6 chained", "bf16" if dt == BF else "fp32")
        _worst[k] = (0.0, max(_worst.get(k, (0, 0))[1], err))
        print(f"[decode_layer_direct] 6 chained c{cluster} t {t}: x_out after two layers worst rel err {err:.3e} (tol {R.OUT_TOL[dt]:.0e})")
        assert err < R.OUT_TOL[dt], (t, err)
    if scratch is not None:
        assert torch.equal(scratch[1][:, 1].cpu(), torch.full((B,), 18, dtype=torch.int32))
