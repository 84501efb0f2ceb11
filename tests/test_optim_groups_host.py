"""Host side of the train step's gradient clipping and parameter groups: argument checks, the group map built from the flat
layout, the HF no-decay split, the C ABI declarations of every optimizer entry point (no GPU)."""
import os
import re

import numpy as np
import pytest

from tests.optim_common import _stub_engine
from vault_amd.params import ParamStore
from vault_amd.spec import VaultSpec, param_entries
from vault_amd.train import TrainStep, build_param_groups, no_decay_parameter_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("groups,match", [
    ([{"params": ["no.such.weight"]}], "unknown parameter"),
    # ViLT's own word table is replaced by the LM's: it never gets a gradient
    ([{"params": ["embeddings.text_embeddings.word_embeddings.weight"]}], "not trained"),
    ([{"params": ["pooler.dense.bias"]}, {"params": ["layernorm.bias", "pooler.dense.bias"]}], "in param_groups"),
    ([{"params": ["pooler.dense.bias", "pooler.dense.bias"]}], "in param_groups"),
    ([{"params": ["pooler.dense.bias"], "betas": (0.9, 0.99)}], "unsupported key"),
    ([{"params": ["pooler.dense.bias"], "eps": 1e-6}], "unsupported key"),
    ([{"params": "pooler.dense.bias"}], "list of parameter names"),
    ([{"lr": 1e-4}], "list of parameter names"),
    ([{"params": ["pooler.dense.bias"], "lr": "fast"}], "not a number"),
    ({"params": ["pooler.dense.bias"]}, "sequence of dicts"),
    ([{"params": []}] * 256, "at most"),
])
def test_param_group_arguments_are_checked(groups, match):
    lay = ParamStore.layout(VaultSpec.tiny(3, "roberta"))
    with pytest.raises(ValueError, match=match):
        build_param_groups(lay, groups, 1e-4, 0.01)
    with pytest.raises(ValueError, match=match):
        TrainStep(_stub_engine(lay), param_groups=groups)


def test_frozen_lm_parameters_are_not_trainable_names():
    lay = ParamStore.layout(VaultSpec.tiny(3, "roberta"), freeze_lm=True)
    with pytest.raises(ValueError, match="not trained"):
        TrainStep(_stub_engine(lay), param_groups=[{"params": ["bert.encoder.layer.0.output.dense.weight"]}])
    build_param_groups(lay, [{"params": ["encoder.layer.0.output.dense.weight"]}], 1e-4, 0.0)     # (ViLT still trains)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_max_grad_norm_must_be_positive(bad):
    lay = ParamStore.layout(VaultSpec.tiny(3, "roberta"))
    with pytest.raises(ValueError, match="max_grad_norm"):
        TrainStep(_stub_engine(lay), max_grad_norm=bad)


def test_group_map_follows_the_flat_layout():
    spec = VaultSpec.tiny(3, "bert")
    lay = ParamStore.layout(spec)
    names_a = ["pooler.dense.weight", "pooler.dense.bias", "bert.embeddings.LayerNorm.bias"]
    names_b = ["encoder.layer.1.intermediate.dense.weight", "classifier.1.bias"]
    gmap, table = build_param_groups(lay, [{"params": names_a, "lr": 3e-4}, {"params": names_b, "weight_decay": 0.0}],
                                     2e-5, 0.01)
    assert gmap.dtype == np.uint8 and gmap.shape == (lay.n_train // 64,)
    np.testing.assert_array_equal(table, np.array([[2e-5, 0.01], [3e-4, 0.01], [2e-5, 0.0]], np.float32))
    want = np.zeros(lay.n_train, np.int64)          # per element, then one entry per 64: every tensor starts 64-aligned
    for k, names in ((1, names_a), (2, names_b)):
        for n in names:
            o, shp = lay.offsets[n]
            assert o % 64 == 0
            want[o:o + int(np.prod(shp))] = k
    for n in lay.trainable:           # every element of a tensor lies in a 64-block of its own group
        o, shp = lay.offsets[n]
        blocks = gmap[o // 64:(o + int(np.prod(shp)) + 63) // 64]
        assert (blocks == want[o]).all(), n
    assert (gmap.astype(np.int64) == want[::64]).all()
    assert set(np.unique(gmap)) == {0, 1, 2}
    # no groups: everything in the default group
    gmap0, table0 = build_param_groups(lay, None, 2e-5, 0.01)
    assert not gmap0.any() and table0.shape == (1, 2)


@pytest.mark.parametrize("kind", ["roberta", "bert"])
def test_no_decay_names_agree_with_the_hf_trainer(kind):
    """The helper's split against transformers' Trainer.get_decay_parameter_names on HF ViLT + RoBERTa / BERT modules of the
    tiny shapes (the LM's names under the ``bert.`` prefix, as in the VAuLT state_dict)."""
    transformers = pytest.importorskip("transformers")
    from oracle.make_goldens import hf_configs
    spec = VaultSpec.tiny(3, kind)
    vc, lc = hf_configs(spec)
    vilt = transformers.ViltModel(vc)
    lm = (transformers.RobertaModel if kind == "roberta" else transformers.BertModel)(lc, add_pooling_layer=False)
    decay = set(transformers.Trainer.get_decay_parameter_names(None, vilt))
    decay |= {"bert." + n for n in transformers.Trainer.get_decay_parameter_names(None, lm)}
    hf_names = [n for n, _ in vilt.named_parameters()] + ["bert." + n for n, _ in lm.named_parameters()]
    ours = [n for n, _, _ in param_entries(spec)]
    assert set(hf_names) <= set(ours)
    no_decay = set(no_decay_parameter_names(spec, hf_names))
    assert no_decay == set(hf_names) - decay
    # the families the issue names are all there
    for n in ("bert.embeddings.LayerNorm.weight", "bert.encoder.layer.0.output.LayerNorm.weight",
              "encoder.layer.1.layernorm_before.weight", "encoder.layer.1.layernorm_after.bias", "layernorm.weight",
              "embeddings.text_embeddings.LayerNorm.weight", "pooler.dense.bias"):
        assert n in no_decay, n
    assert "pooler.dense.weight" not in no_decay and "embeddings.cls_token" not in no_decay


def test_no_decay_names_see_the_mlp_heads_layernorm_by_module():
    spec = VaultSpec.tiny(3, "roberta")
    spec.head = "mlp"
    names = [n for n, _, _ in param_entries(spec) if n.startswith("classifier.")]
    assert sorted(no_decay_parameter_names(spec, names)) == ["classifier.0.bias", "classifier.1.bias", "classifier.1.weight",
                                                             "classifier.3.bias"]


_TORCH_PARAMS = ["float* p", "float* g", "float* m", "float* v", "void* p_bf16", "float* ema", "long long n",
                 "const unsigned char* group_map", "const float* group_table", "int n_groups", "float lr_factor",
                 "float beta1", "float beta2", "float eps", "float inv_bias_corr1", "float inv_sqrt_bias_corr2",
                 "float grad_scale", "const float* coef", "float one_minus_decay", "int zero_grad",
                 "const unsigned char* zero_mask", "void* stream"]


# (symbol of include/vault_hip.h, its name in ops, the parameters its declaration starts with - all of them for the torch form)
_DECLARED = [("vault_grad_norm", "grad_norm", None),
             ("VAULT_GRAD_NORM_PARTIALS", "GRAD_NORM_PARTIALS", None),
             ("vault_adamw_step_grouped", "adamw_step_grouped", None),
             ("vault_adamw_step_ema", "adamw_step_ema", _TORCH_PARAMS[:7]),
             ("vault_ema_swap", "ema_swap", None),
             ("vault_adamw_step_torch", "adamw_step_torch", _TORCH_PARAMS)]


@pytest.mark.parametrize("symbol,wrapper,params", _DECLARED, ids=[d[0] for d in _DECLARED])
def test_optimizer_entry_points_are_declared_and_wrapped(symbol, wrapper, params):
    from vault_amd import ops
    hdr = open(os.path.join(ROOT, "include", "vault_hip.h")).read()
    if symbol.isupper():
        m = re.search(r"#define\s+" + symbol + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(ops, wrapper)
        return
    assert re.search(r"\bint\s+" + symbol + r"\s*\(", hdr), symbol
    assert callable(getattr(ops, wrapper))
    if params is not None:
        m = re.search(r"\bint\s+" + symbol + r"\s*\((.*?)\)\s*;", hdr, re.S)
        assert m
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        args = [re.sub(r"\s+", " ", a_).strip() for a_ in args.split(",")]
        assert args[:len(params)] == params and (params is not _TORCH_PARAMS or args == params)
