"""Host side of the train step's weight average and resumable optimizer state: the decay schedule, the validation of a saved
state against the flat layout, and the option's argument check (no GPU; the C ABI declarations: tests/test_optim_groups_host.py)."""
import pytest
import torch

from tests.optim_common import _stub_engine
from vault_amd.params import ParamStore
from vault_amd.spec import VaultSpec
from vault_amd.train import TrainStep, check_optimizer_state, ema_decay_at


def test_ema_decay_without_warmup_is_constant():
    for d in (0.0, 0.5, 0.9, 0.9999):
        assert {ema_decay_at(d, t, False) for t in (1, 2, 10, 1000, 10 ** 7)} == {d}
        assert ema_decay_at(d, 3) == d                                    # (warm-up is opt-in)


def test_ema_decay_warmup_ramps_to_the_decay():
    assert ema_decay_at(0.9, 1, True) == 2.0 / 11.0
    assert ema_decay_at(0.9999, 1, True) == 2.0 / 11.0
    d = 0.9
    # (1 + t) / (10 + t) > 0.9  <=>  t > 80: the ramp until then, the decay afterwards
    for t in range(1, 200):
        ramp = (1.0 + t) / (10.0 + t)
        want = ramp if ramp <= d else d
        assert ema_decay_at(d, t, True) == want, t
    assert ema_decay_at(d, 80, True) == 81.0 / 90.0 and ema_decay_at(d, 81, True) == d
    assert ema_decay_at(0.1, 1, True) == 0.1                              # a decay below the ramp's start holds at once
    vals = [ema_decay_at(0.999, t, True) for t in range(1, 20000)]
    assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[-1] == 0.999


def _good_state(lay, ema=True):
    part = lambda: {n: torch.zeros(lay.offsets[n][1]) for n in lay.trainable}  # noqa: E731
    return {"step_idx": 2, "drop_seed": 7, "exp_avg": part(), "exp_avg_sq": part(), "ema": part() if ema else None,
            "hyper": {"lr": 1.0, "betas": (0.5, 0.5), "eps": 1.0, "weight_decay": 3.0, "correct_bias": True,
                      "total_steps": 1, "warmup_steps": 1, "ema_decay": 0.123, "ema_warmup": True}}


@pytest.fixture(params=[False, True], ids=["train_lm", "freeze_lm"])
def lay(request):
    return ParamStore.layout(VaultSpec.tiny(3, "roberta"), freeze_lm=request.param)


def test_check_optimizer_state_accepts_a_well_formed_dict(lay):
    check_optimizer_state(lay, _good_state(lay, True), True)
    check_optimizer_state(lay, _good_state(lay, False), False)      # (the hyper-parameters in it are not compared)
    sd = _good_state(lay, False)
    del sd["hyper"]
    check_optimizer_state(lay, sd, False)


@pytest.mark.parametrize("key", ["exp_avg", "exp_avg_sq", "ema"])
def test_check_optimizer_state_names_and_shapes(lay, key):
    some = "pooler.dense.weight"
    assert some in lay.trainable
    sd = _good_state(lay)
    sd[key]["no.such.weight"] = torch.zeros(3)
    with pytest.raises(ValueError, match="unknown parameter"):
        check_optimizer_state(lay, sd, True)
    # ViLT's own word table is replaced by the LM's: it never gets a gradient, so it has no optimizer state
    sd = _good_state(lay)
    frozen = "embeddings.text_embeddings.word_embeddings.weight"
    assert frozen in lay.frozen
    sd[key][frozen] = torch.zeros(lay.offsets[frozen][1])
    with pytest.raises(ValueError, match="not trained"):
        check_optimizer_state(lay, sd, True)
    sd = _good_state(lay)
    del sd[key][some]
    with pytest.raises(ValueError, match="lacks"):
        check_optimizer_state(lay, sd, True)
    sd = _good_state(lay)
    sd[key][some] = sd[key][some].reshape(-1)                             # the right count in the wrong shape
    with pytest.raises(ValueError, match="shape"):
        check_optimizer_state(lay, sd, True)
    sd = _good_state(lay)
    sd[key][some] = sd[key][some][:-1]
    with pytest.raises(ValueError, match="shape"):
        check_optimizer_state(lay, sd, True)


def test_check_optimizer_state_ema_presence(lay):
    with pytest.raises(ValueError, match="weight average"):
        check_optimizer_state(lay, _good_state(lay, True), False)
    with pytest.raises(ValueError, match="no weight average"):
        check_optimizer_state(lay, _good_state(lay, False), True)
    sd = _good_state(lay)
    del sd["exp_avg_sq"]
    with pytest.raises(ValueError, match="lacks"):
        check_optimizer_state(lay, sd, True)
    with pytest.raises(ValueError, match="must be a dict"):
        check_optimizer_state(lay, [1, 2], True)


def test_check_optimizer_state_refuses_lm_names_under_freeze_lm():
    full = ParamStore.layout(VaultSpec.tiny(3, "roberta"))
    frozen = ParamStore.layout(VaultSpec.tiny(3, "roberta"), freeze_lm=True)
    sd = _good_state(full)                                               # a state saved by a run that trained the LM
    assert any(n.startswith("bert.") for n in sd["exp_avg"])
    with pytest.raises(ValueError, match=r"'bert\..*not trained"):
        check_optimizer_state(frozen, sd, True)
    sd = _good_state(frozen)
    sd["ema"]["bert.encoder.layer.0.output.dense.weight"] = torch.zeros(
        frozen.offsets["bert.encoder.layer.0.output.dense.weight"][1])
    with pytest.raises(ValueError, match="not trained"):
        check_optimizer_state(frozen, sd, True)
    # and the other way round: the frozen run's state lacks the LM's moments
    with pytest.raises(ValueError, match="lacks"):
        check_optimizer_state(full, _good_state(frozen), True)


@pytest.mark.parametrize("decay", [1.0, -0.1, 1.5, float("nan")])
def test_ema_decay_outside_the_unit_interval_is_refused(decay):
    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(_stub_engine(), ema_decay=decay)
