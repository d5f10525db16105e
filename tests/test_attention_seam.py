"""CPU checks of the third operator seam, MultiheadAttention.forward of resblocks[i].attn (reference model.py:837-944): the
library exports its entry points, the mirror's ``attn`` child is callable with the reference's signature, the restrictions of
the engine's form are refused with errors that name them before anything touches the engine, and the parameter names and
their order are those of the reference.  The GPU side is tests/test_gpu_attention_seam.py."""
import inspect
import os

import pytest
import torch
from torch import nn

from conftest import load_golden, load_tiny_sd

from pevit_amd import _lib
from pevit_amd.evaluation.model import build_peft_model

METHODS = ["kadaptation", "lora", "adapter", "compacter"]
FIXTURES = ["tiny_kadaptation", "tiny_lora", "tiny_lora_r8", "tiny_adapter", "tiny_compacter"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module", params=METHODS)
def model(request):
    return build_peft_model(load_tiny_sd(), request.param)


def test_library_exports_the_attention_seam(lib):
    for name in ("pevit_attention_forward", "pevit_attention_backward", "pevit_op_attn_probs"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_attn_is_callable_with_the_reference_signature(model):
    attn = model.visual.transformer.resblocks[0].attn
    assert type(attn).forward is not nn.Module.forward
    sig = inspect.signature(type(attn).forward)
    params = list(sig.parameters.values())
    assert [p.name for p in params] == ["self", "query", "key", "value", "key_padding_mask", "need_weights", "attn_mask",
                                        "average_attn_weights"]
    defaults = {p.name: p.default for p in params if p.default is not inspect.Parameter.empty}
    assert defaults == {"key_padding_mask": None, "need_weights": True, "attn_mask": None, "average_attn_weights": True}
    assert attn.embed_dim == 128 and attn.num_heads == 2 and attn.batch_first is False
    for blk in model.visual.transformer.resblocks:
        assert type(blk.attn) is type(attn)


def _x(model, n=None, b=3):
    E = model.visual.arch.width
    return torch.randn(n or model.visual.arch.tokens, b, E)


def test_cross_attention_is_refused_on_cpu(model):
    attn = model.visual.transformer.resblocks[1].attn
    x, y = _x(model), _x(model)
    with pytest.raises(_lib.PevitError, match="query, key and value must be the same tensor"):
        attn(x, y, y)
    with pytest.raises(_lib.PevitError, match="query, key and value must be the same tensor"):
        attn(x, x, x.clone())
    with pytest.raises(_lib.PevitError, match="query, key and value must be the same tensor"):
        attn(x, x[:, :2], x)


def test_masks_are_refused_on_cpu(model):
    attn = model.visual.transformer.resblocks[0].attn
    x = _x(model)
    N = x.shape[0]
    with pytest.raises(_lib.PevitError, match="attn_mask must be None"):
        attn(x, x, x, attn_mask=torch.zeros(N, N))
    with pytest.raises(_lib.PevitError, match="key_padding_mask must be None"):
        attn(x, x, x, key_padding_mask=torch.zeros(x.shape[1], N, dtype=torch.bool))


def test_input_geometry_is_refused_on_cpu(model):
    attn = model.visual.transformer.resblocks[0].attn
    bad = [_x(model, n=model.visual.arch.tokens + 1), _x(model).permute(1, 0, 2), _x(model)[0],
           torch.randn(model.visual.arch.tokens, 3, 64)]
    for x in bad:
        with pytest.raises(_lib.PevitError, match=r"must be 3-D \(N, B, E\)"):
            attn(x, x, x)


def test_a_valid_call_reaches_the_engine_error_on_cpu(model):
    """Same tensor passed three times, or three views of one buffer: validation passes, and the CPU-resident module then
    refuses to run outside the HIP engine (there is no PyTorch fallback)."""
    attn = model.visual.transformer.resblocks[0].attn
    x = _x(model)
    with pytest.raises(_lib.PevitError, match="runs only in the HIP engine"):
        attn(x, x, x)
    with pytest.raises(_lib.PevitError, match="runs only in the HIP engine"):
        attn(x, x.view_as(x), x[:], need_weights=False)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_named_parameters_unchanged(fixture):
    meta, _ = load_golden(fixture)
    m = build_peft_model(load_tiny_sd(), meta["method"], meta["lora_r"])
    assert [n for n, _ in m.named_parameters()] == meta["all_names"]
    attn_names = [n for n, _ in m.visual.transformer.resblocks[0].attn.named_parameters()]
    pre = "visual.transformer.resblocks.0.attn."
    assert attn_names == [n[len(pre):] for n in meta["all_names"] if n.startswith(pre)]
