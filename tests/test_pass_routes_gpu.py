"""Which launches a pass is made of (csrc/m3pc_passes.hip), pinned by the library's own profile brackets.

A change of the host code that sends a shape to the GEMM chain instead of the fused layer tail passes every tolerance test -- the
chain gives the same numbers to within bf16 -- and shows only as a slower bench shape.  So the route is pinned: with
``profile_enable(True)`` every matrix-core launch of a call sits in a bracket that carries its algorithmic flops, and the count
and flop sum of the brackets (integers below 2^53, exact in a double) name the route.  Three reads per call: the fused layer
tails alone (``PROF_LAYER_TAIL``), the launches in the pass's own arithmetic, and all of them.

The literals are what the library computed before the pass code was restructured; each carries the routing rule it follows from.
d = 512, ff = 2048, ``Dims(11, 3, 32)`` with H = 16: Le = 49 encoder tokens per candidate, of which 33 are history (32 of them
stored once, the first layer's shared rows), and 2 H = 32 decoder query rows.  Thresholds (m3pc_internal.h): the full fused tail
from 96 * 128 = 12288 rows of the whole step, the split tail from 16 * 128 = 2048, below that the GEMM chain."""
import pytest
import torch

from m3pc_amd import capi, synth
from hip_util import make_handle, window_dev
from oracle import mtm_oracle as O

pytestmark = pytest.mark.gpu
BF16, FP32 = capi.PREC_BF16, capi.PREC_FP32
D, FF = 512, 2048
TAIL = 2 * (D * D + 2 * D * FF)  # flops per row of a layer tail: out-proj + linear1 + linear2
QKV = 2 * 3 * D * D              # ... of a Q|K|V projection (also: the decoder's embedding + K|V inside kv_fused)
DD = 2 * D * D                   # ... of one d x d GEMM


def _setup(dims, H, n_max):
    h, *_ = make_handle(dims, max_candidates=n_max, max_batch=1)
    cfg = O.PlanCfg(dims.traj_length, H, n_max)
    win, _ = O.assemble_window(cfg, synth.make_history(dims, 0), 500, 3.0)
    eps = synth.make_eps(n_max, dims, 1)[:, 0, :, 0, :].cuda()
    return h, window_dev(win), eps


@pytest.fixture(scope="module")
def big():
    """One handle at T = 32 for every case but the shipped small config."""
    h, win, eps = _setup(synth.Dims(11, 3, 32), 16, 384)
    yield h, win, eps
    h.close()


def _profiled(h, prec, call):
    """call() once un-profiled (the cached tables of the plan are built outside the brackets), once profiled ->
    (result, {"tail" | "own" | "all": (launches, flops)})."""
    call()
    h.profile_read(-1)
    h.profile_enable(True)
    out = call()
    got = {}
    for name, which in (("tail", capi.PROF_LAYER_TAIL), ("own", prec), ("all", -1)):
        n, _, fl = h.profile_read(which, reset=which == -1)
        assert fl == int(fl)
        got[name] = (n, int(fl))
    h.profile_enable(False)
    return out, got


def _step(h, win, eps, mode, N, H=16, prec=BF16, **kw):
    s, a, r = win
    return lambda: h.plan_step(mode, s, a, r, eps[:N].contiguous(), H, 3.0, 0.6, 0.99, N, precision=prec, **kw)["expect_return"].clone()


def _check(case, got, want):
    print(case, got)
    assert got == want, (case, got, want)


# The fp32 policy pass in front of every plan step (the generic forward on one sequence): 13 launches = 2 encoder layers x 4 GEMMs
# over the 65 kept tokens (T = 8: 17), the four decoder embeddings as one grouped launch, the decoder layer's 4 GEMMs over 4 T rows.
POLICY_T32 = (13, 1690304512)  # 2 * 65 * (QKV + TAIL) + 128 * DD + 128 * (QKV + TAIL)
POLICY_T8 = (13, 432013312)    # 2 * 17 * (QKV + TAIL) + 32 * DD + 32 * (QKV + TAIL)
assert POLICY_T32[1] == 2 * 65 * (QKV + TAIL) + 128 * DD + 128 * (QKV + TAIL) and POLICY_T8[1] == 2 * 17 * (QKV + TAIL) + 32 * DD + 32 * (QKV + TAIL)


def _with_policy(own, policy):
    return (own[0] + policy[0], own[1] + policy[1])


# case -> the three reads.  LayerNorm, attention, embedding, gather and head-output launches carry no bracket.
EXPECT = {
    # N = 256: 12544 encoder rows >= 12288 -> both encoder tails full, the first with the second layer's Q|K|V inside (the bf16
    # residual stream needs that consumer); 8192 decoder rows -> split tail (its reduce is no bracket), heads as launches.
    "rtg256": dict(
        tail=(3, 176764747776),   # 12544 * (TAIL + QKV) + 12544 * TAIL + 8192 * TAIL
        own=(8, 207685156864),    # tails + layer-0 Q|K|V of the 256 * 17 own rows + of the 32 shared rows (the compact shared block)
                                  # + embedding + K|V of the decoder in one launch (12544 * QKV) + 2 head GEMMs (4096 * DD each)
        all=_with_policy((8, 207685156864), POLICY_T32)),
    # N = 384: 12288 decoder rows, exactly the threshold -> full tail with both scalar heads inside (+ DD per row), no head launch
    "rtg384": dict(
        tail=(3, 271589572608),   # 18816 * (TAIL + QKV) + 18816 * TAIL + 12288 * (TAIL + DD)
        own=(6, 311502569472),    # tails + Q|K|V of 384 * 17 own + 32 shared rows + 18816 * QKV (decoder embedding + K|V)
        all=_with_policy((6, 311502569472), POLICY_T32)),
    # critic, N = 384: the states head is no scalar head -> full tail writes the heads' LayerNorm rows, 2 head GEMMs (6144 * DD each);
    # one query token per candidate is un-masked (the mix prefix): its decoder embedding and Q projection are GEMMs of 384 rows
    "critic384": dict(
        tail=(3, 265147121664),   # 18816 * (TAIL + QKV) + 18816 * TAIL + 12288 * TAIL
        own=(10, 311905222656),   # tails + the 3 launches of rtg384 + 384 * (DD + DD) + 2 * 6144 * DD
        all=_with_policy((10, 311905222656), POLICY_T32)),
    # N = 64: 3136 encoder rows and 2048 decoder rows (exactly the lower threshold) -> three split tails; no Q|K|V inside a split
    # tail, so the second layer's projection is a GEMM of 3136 rows; 64 candidates still share the 32 history rows of layer 0
    "rtg64": dict(
        tail=(3, 39258685440),    # (3136 + 3136 + 2048) * TAIL
        own=(9, 51959037952),     # tails + (64 * 17 + 32 + 3136) * QKV + 3136 * QKV (decoder embedding + K|V) + 2 * 1024 * DD
        all=_with_policy((9, 51959037952), POLICY_T32)),
    # N = 32: 1568 / 1024 rows -> the GEMM chain everywhere (and fewer than 64 candidates: no shared rows): 2 x 4 encoder GEMMs,
    # decoder embedding + K|V in one launch (1568 rows >= 512), out-proj / linear1 / linear2, 2 head GEMMs
    "rtg32": dict(
        tail=(0, 0),
        own=(14, 27564965888),    # 2 * 1568 * (QKV + TAIL) + 1568 * QKV + 1024 * TAIL + 2 * 512 * DD
        all=_with_policy((14, 27564965888), POLICY_T32)),
    # the shipped small config: Le = 13, 8 query rows; 8125 / 5000 rows -> three split tails, two full-row Q|K|V GEMMs
    "rtg625_T8": dict(
        tail=(3, 100270080000),   # (8125 + 8125 + 5000) * TAIL
        own=(8, 141230080000),    # tails + 2 * 8125 * QKV + 8125 * QKV (decoder embedding + K|V) + 2 * 2500 * DD
        all=_with_policy((8, 141230080000), POLICY_T8)),
    # fp32 re-score of 16: 784 / 512 rows, the chain (its LayerNorms ride on the split-K reduces: no bracket either way): 2 x 4 encoder
    # GEMMs, the two kept keys' decoder embeddings as one grouped launch, K|V, out-proj / linear1 / linear2, both scalar heads in one
    "rescore16": dict(
        tail=(0, 0),
        own=(14, 13782482944),    # 2 * 784 * (QKV + TAIL) + 784 * DD + 784 * 2 * DD + 512 * TAIL + 2 * 256 * DD
        all=(14, 13782482944)),
    # the candidate pass of N = 256 alone: rtg256 without the policy pass
    "cand256": dict(tail=(3, 176764747776), own=(8, 207685156864), all=(8, 207685156864)),
}


def test_rtg_256_full_encoder_split_decoder(big):
    h, win, eps = big
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_RTG, 256))
    _check("rtg256", got, EXPECT["rtg256"])


def test_rtg_384_full_decoder_tail_with_scalar_heads(big):
    h, win, eps = big
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_RTG, 384))
    _check("rtg384", got, EXPECT["rtg384"])


def test_critic_384_mix_prefix_through_the_fused_tail(big):
    h, win, eps = big
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_CRITIC, 384))
    _check("critic384", got, EXPECT["critic384"])


def test_rtg_64_split_tails(big):
    h, win, eps = big
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_RTG, 64))
    _check("rtg64", got, EXPECT["rtg64"])


def test_rtg_32_gemm_chain(big):
    h, win, eps = big
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_RTG, 32))
    _check("rtg32", got, EXPECT["rtg32"])


def test_shipped_small_config_625():
    """N = 625, T = 8, H = 4: Le = 13 with 9 history tokens -- fewer than one 32-row tile, so no shared rows."""
    h, win, eps = _setup(synth.Dims(11, 3, 8), 4, 625)
    _, got = _profiled(h, BF16, _step(h, win, eps, capi.MODE_RTG, 625, H=4))
    h.close()
    _check("rtg625_T8", got, EXPECT["rtg625_T8"])


def test_fp32_rescore_of_16(big):
    h, win, eps = big
    s, a, r = win
    _step(h, win, eps, capi.MODE_RTG, 256)()  # the step that owns slot 0
    index = torch.arange(3, 256, 16, dtype=torch.int32, device="cuda")
    assert index.numel() == 16
    _, got = _profiled(h, FP32, lambda: h.rescore(capi.MODE_RTG, s, a, r, eps[:256].contiguous(), index, 16, 3.0, 0.6, 0.99, 256)[0].clone())
    _check("rescore16", got, EXPECT["rescore16"])


def test_two_shards_take_the_routes_of_the_whole(big):
    """The choice goes by the size of the whole step: two shards of 128 launch what N = 256 launches, twice, over the same rows."""
    h, win, eps = big
    s, a, r = win
    e = eps[:256].contiguous()
    h.policy_pass(capi.MODE_RTG, s, a, r, 16, 3.0)

    def cand(b, n):
        return lambda: h.candidate_pass(capi.MODE_RTG, s, a, r, e, 16, 0.6, 0.99, 256, n_begin=b, n_count=n, precision=BF16)["expect_return"].clone()

    whole, gw = _profiled(h, BF16, cand(0, 256))
    p0, g0 = _profiled(h, BF16, cand(0, 128))
    p1, g1 = _profiled(h, BF16, cand(128, 128))
    print("shards", gw, g0, g1)
    assert torch.equal(whole, torch.cat([p0, p1]))
    assert g0 == g1
    for k in ("tail", "own", "all"):
        assert g0[k][0] + g1[k][0] == 2 * gw[k][0], (k, gw, g0, g1)
    assert g0["tail"][1] + g1["tail"][1] == gw["tail"][1]
    # every other launch is per candidate row too, but for the Q|K|V projection of the 32 shared history rows, which each shard runs
    assert g0["own"][1] + g1["own"][1] == gw["own"][1] + 32 * QKV
    _check("cand256", gw, EXPECT["cand256"])
