"""The embedding kernel (embed_rows_kernel, csrc/elementwise.hip) storing the bf16 residual rows compactly (EmbedP::x_compact): the
n_indep history rows once, then every candidate's own rows -- the block the first layer's fused tail reads (block_res_row_xb).
Against the same launch in the full layout (every candidate all of its L rows), through the lab hook m3pc_debug_embed: the shared
block is candidate 0's leading rows, every compact own row is its full-layout row, and the LayerNorm rows (Hb / Hb_sh) do not
change -- bit for bit, since the arithmetic is the same and only the store address differs."""
import ctypes as C

import pytest
import torch

from hip_util import lab_library

pytestmark = pytest.mark.gpu

DEV, BF, SENT = "cuda", torch.bfloat16, -31744.0
D, T, L, N_INDEP, N_SH = 512, 32, 49, 33, 32
FEAT = (11, 3)
vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong


class EArgs(C.Structure):
    """m3pc_debug_embed_args (include/m3pc_hip_debug.h)."""
    _fields_ = [("tok", vp * 4), ("bstride", ll * 4), ("WT", vp * 4), ("E", vp * 4), ("feat", ci * 4), ("tokmap", vp), ("batch", ci),
                ("L", ci), ("d", ci), ("T", ci), ("X", vp), ("Xb", vp), ("ln_g", vp), ("ln_b", vp), ("Hb", vp), ("Hb_sh", vp),
                ("n_indep", ci), ("n_sh", ci), ("x_first_only", ci), ("x_compact", ci), ("stream", vp)]


@pytest.fixture(scope="module")
def lib():
    lib = lab_library()
    lib.m3pc_debug_embed.restype, lib.m3pc_debug_embed.argtypes = ci, [C.POINTER(EArgs)]
    return lib


@pytest.fixture(scope="module")
def model():
    g = torch.Generator(device=DEV).manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    # 17 states, the 16 history actions, then the candidate's own 16 actions
    tokmap = torch.tensor([[0, t] for t in range(17)] + [[1, t] for t in range(32)], dtype=torch.int32, device=DEV)
    return dict(WT=[rn(f, D) for f in FEAT], E=[rn(T, D) for _ in FEAT], g=1 + 0.1 * rn(D), b=0.1 * rn(D), tokmap=tokmap,
                states=rn(T, FEAT[0]), hist=rn(16, FEAT[1]))


def _run(lib, m, batch, actions, compact):
    n_own = L - N_INDEP
    xrows = N_INDEP + batch * n_own if compact else batch * L
    Xb = torch.full((xrows + 1, D), SENT, device=DEV, dtype=BF)
    Hb = torch.full((batch * (L - N_SH) + 1, D), SENT, device=DEV, dtype=BF)
    Hs = torch.full((N_SH + 1, D), SENT, device=DEV, dtype=BF)
    a = EArgs()
    a.tok = (vp * 4)(m["states"].data_ptr(), actions.data_ptr(), None, None)
    a.bstride = (ll * 4)(0, T * FEAT[1], 0, 0)
    a.WT = (vp * 4)(m["WT"][0].data_ptr(), m["WT"][1].data_ptr(), None, None)
    a.E = (vp * 4)(m["E"][0].data_ptr(), m["E"][1].data_ptr(), None, None)
    a.feat = (ci * 4)(FEAT[0], FEAT[1], 0, 0)
    a.tokmap, a.batch, a.L, a.d, a.T = m["tokmap"].data_ptr(), batch, L, D, T
    a.Xb, a.ln_g, a.ln_b, a.Hb, a.Hb_sh = Xb.data_ptr(), m["g"].data_ptr(), m["b"].data_ptr(), Hb.data_ptr(), Hs.data_ptr()
    a.n_indep, a.n_sh, a.x_first_only, a.x_compact = N_INDEP, N_SH, int(compact), int(compact)
    a.stream = torch.cuda.current_stream().cuda_stream
    assert lib.m3pc_debug_embed(C.byref(a)) == 0, lib.m3pc_last_error()
    torch.cuda.synchronize()
    return Xb, Hb, Hs


def _bits(t):
    return t.contiguous().view(torch.int16)


# (batch < 128: one batch element per wave; 131 / 512: chunks of 2 / 8 elements per wave -- the wave then re-stores a shared token's
# values for every element of its chunk in the full layout and must store them for element 0 alone in the compact one -- 131 with a
# ragged last chunk, 512 the half of the headline pass)
@pytest.mark.parametrize("batch", [1, 3, 17, 131, 512])
def test_compact_rows_are_the_full_layout_rows(lib, model, batch):
    g = torch.Generator(device=DEV).manual_seed(batch)
    actions = torch.randn(batch, T, FEAT[1], device=DEV, generator=g)
    actions[:, :16] = model["hist"]  # (the history: the same for every candidate)
    Xf, Hf, Hsf = _run(lib, model, batch, actions, False)
    Xc, Hc, Hsc = _run(lib, model, batch, actions, True)
    n_own = L - N_INDEP
    full = Xf[:batch * L].view(batch, L, D)
    assert not bool((full == SENT).any()) and bool(torch.isfinite(full.float()).all())
    assert bool((Xf[batch * L] == SENT).all())
    # (what makes storing them once legitimate)
    assert torch.equal(_bits(full[:, :N_INDEP]), _bits(full[:1, :N_INDEP].expand(batch, N_INDEP, D)))
    assert torch.equal(_bits(Xc[:N_INDEP]), _bits(full[0, :N_INDEP])), "the shared block is not candidate 0's leading rows"
    own = Xc[N_INDEP:N_INDEP + batch * n_own].view(batch, n_own, D)
    assert torch.equal(_bits(own), _bits(full[:, N_INDEP:])), "a compact own row differs from its full-layout row"
    assert bool((Xc[N_INDEP + batch * n_own] == SENT).all()), "a row behind the compact block was written"
    assert torch.equal(_bits(Hc), _bits(Hf)) and torch.equal(_bits(Hsc), _bits(Hsf)), "the LayerNorm rows changed"
    assert not bool((Hf[:-1] == SENT).any()) and not bool((Hsf[:-1] == SENT).any())
