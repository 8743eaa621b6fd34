"""The mode keywords of MLA.predict_action_diff* in combination: which keyword a call refuses (and with which exception class), which
combinations get past the argument checks, what a shape no engine serves raises, and which keywords a call that ends in another public
method hands on. The other host tests pin one keyword at a time; these pin pairs.

The expected outcomes in tests/golden/sampling_mode_outcomes.json were recorded from the commit BEFORE the mode plumbing was folded into
infer.MODES (`PYTHONPATH=. python tests/test_sampling_modes_host.py --record` there), never from the code under test: the file is a table of the
distinct outcomes and one index per generated case, in generation order. Only the public methods are called; the stand-in `self` hands
every attribute it lacks to the MLA function of that name bound to itself, so the private helpers are free to change."""
import inspect
import itertools
import json
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

from mla_amd.mla import MLA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_mode_outcomes.json")

# keyword -> its non-default values, in the public methods' order; "bogus" is added where the unknown value is part of the case
VALUES = {"suffix_weights": ("fp8", "fp8_as_bf16"), "prefill": ("compact",), "sampler": ("device",), "suffix_attention": ("split",),
          "prefill_precision": ("fp8", "fp8_as_bf16"), "groups_attention": ("split",), "batch_prefill": ("fp8", "fp8_as_bf16"),
          "ddpm_sampler": ("device",), "suffix_operand": ("once",)}
NAME = re.compile(r"\b(" + "|".join(VALUES) + r")\b")
SINGLE = [k for k in VALUES if k not in ("groups_attention", "batch_prefill")]           # predict_action_diff
SAMPLES = [k for k in VALUES if k != "batch_prefill"]                                   # predict_action_diff_samples
BATCH = list(VALUES)                                                                     # predict_action_diff_batch
DDIM = [{"use_ddim": True, "num_ddim_steps": 8}, {"use_ddim": False, "num_ddim_steps": 8}, {"use_ddim": True, "num_ddim_steps": None}]
T = 16                                                                                   # future_action_window_size + 1


class StandIn(types.SimpleNamespace):
    """`self` without a model: an attribute it lacks is the MLA function of that name, bound to it."""

    def __getattr__(self, name):
        try:
            attr = inspect.getattr_static(MLA, name)
        except AttributeError:
            raise AttributeError(name) from None
        if isinstance(attr, staticmethod):
            return attr.__func__
        if inspect.isfunction(attr):
            return types.MethodType(attr, self)
        raise AttributeError(name)


def settings(names, bogus):
    """{} (the defaults), every keyword set singly to each value, every pair of keywords over the same values."""
    values = {k: VALUES[k] + (("bogus",) if bogus else ()) for k in names}
    out = [{}] + [{k: v} for k in names for v in values[k]]
    for a, b in itertools.combinations(names, 2):
        out += [{a: va, b: vb} for va in values[a] for vb in values[b]]
    return out


def outcome(call, serve=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                       # the warned loops of a shape no engine serves
        try:
            call()
        except (ValueError, NotImplementedError) as e:
            m = NAME.search(str(e))
            return [type(e).__name__, m.group(1) if m else None] + (["does not serve" in str(e)] if serve else [])
        except AttributeError:
            return "validated"
    return "returned"                                                         # the forwarding part's recorders only


def model(head_dim=64, **attrs):
    cfg = types.SimpleNamespace(hidden_size=4 * head_dim, num_attention_heads=4)
    vlm = types.SimpleNamespace(llm_backbone=types.SimpleNamespace(llm=types.SimpleNamespace(config=cfg)))
    return StandIn(future_action_window_size=T - 1, _check_cfg_scale=lambda cfg_scale: None, vlm=vlm, **attrs)


def batch_args(B):
    return {"input_ids": [torch.tensor([1, 5 + b, 29871]) for b in range(B)], "cur_robot_states": [0] * B}


def grid_cases():
    """Part 1: the argument checks alone, on a stand-in with nothing in it."""
    routes = [("diff", SINGLE, lambda s, kw: MLA.predict_action_diff(s, **kw)),
              ("samples[1]", SAMPLES, lambda s, kw: MLA.predict_action_diff_samples(s, num_samples=1, **kw)),
              ("samples[3]", SAMPLES, lambda s, kw: MLA.predict_action_diff_samples(s, num_samples=3, **kw)),
              ("batch[1]", BATCH, lambda s, kw: MLA.predict_action_diff_batch(s, [None], [None], **kw)),
              ("batch[2]", BATCH, lambda s, kw: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, **kw)),
              ("batch[2x2]", BATCH, lambda s, kw: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, num_samples=2, **kw))]
    for name, names, call in routes:
        for reuse in (True, False):
            for ddim in DDIM:
                for kw in settings(names, bogus=True):
                    yield (name, reuse, ddim, kw), outcome(lambda: call(StandIn(), dict(kw, reuse_prefix=reuse, **ddim)))


def unserved_cases():
    """Part 2: head_dim 64, which no engine serves, on the routes with more than one chunk per call."""
    routes = [("samples[3]", SAMPLES, lambda s, kw: MLA.predict_action_diff_samples(s, num_samples=3, **kw)),
              ("batch[2]", BATCH, lambda s, kw: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, **batch_args(2), **kw)),
              ("batch[2x2]", BATCH, lambda s, kw: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, num_samples=2, **batch_args(2), **kw))]
    for name, names, call in routes:
        for ddim in DDIM:
            for kw in settings(names, bogus=False):
                yield (name, ddim, kw), outcome(lambda: call(model(64), dict(kw, reuse_prefix=True, **ddim)), serve=True)


def forwarding_cases():
    """Part 3: the keyword dicts a route hands to predict_action_diff / predict_action_diff_samples, one list per case (or what the
    route raises instead). Values that are no plain settings are recorded by their type."""
    def forwarded(call, head_dim, kw):
        calls = []

        def recorder(name):
            def rec(*args, **inner):
                calls.append([name, {k: v if isinstance(v, (str, bool, int, type(None))) else type(v).__name__ for k, v in inner.items()}])
                return np.zeros((1, T, 7))
            return rec
        s = model(head_dim, predict_action_diff=recorder("predict_action_diff"),
                  predict_action_diff_samples=recorder("predict_action_diff_samples"))
        return [calls, outcome(lambda: call(s, kw))]

    def batch(B, **fixed):
        return lambda s, kw: MLA.predict_action_diff_batch(s, [None] * B, [None] * B, **batch_args(B), **fixed, **kw)

    def samples(N):
        return lambda s, kw: MLA.predict_action_diff_samples(s, num_samples=N, input_ids=torch.tensor([[1, 29871]]), **kw)
    # (route, keywords, call, head_dim, reuse_prefix)
    routes = [("batch[1]", BATCH, batch(1), 128, True), ("batch[1xN]", BATCH, batch(1, num_samples=2), 128, True),
              ("samples[1]", SAMPLES, samples(1), 128, True),
              ("batch[2] off", BATCH, batch(2), 128, False), ("batch[2x2] off", BATCH, batch(2, num_samples=2), 128, False),
              ("samples[3] off", SAMPLES, samples(3), 128, False),
              ("batch[2] unserved", BATCH, batch(2), 64, True), ("batch[2x2] unserved", BATCH, batch(2, num_samples=2), 64, True),
              ("samples[3] unserved", SAMPLES, samples(3), 64, True),
              ("batch[2x16] beyond a pass", BATCH, batch(2, num_samples=16), 128, True)]   # 16 groups of 17 rows > 256
    for name, names, call, head_dim, reuse in routes:
        for ddim in DDIM:
            for kw in [{}] + [{k: v} for k in names for v in VALUES[k]]:
                yield (name, ddim, kw), forwarded(call, head_dim, dict(kw, reuse_prefix=reuse, **ddim))


PARTS = {"grid": grid_cases, "unserved": unserved_cases, "forwarding": forwarding_cases}


def run(part):
    return [(case, json.loads(json.dumps(result))) for case, result in PARTS[part]()]


@pytest.mark.parametrize("part", list(PARTS))
def test_outcomes_are_the_recorded_ones(part):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = run(part)
    assert len(got) == len(golden[part]), "the generated cases are the recorded ones, none dropped"
    wrong = [(case, result, golden["outcomes"][i]) for (case, result), i in zip(got, golden[part]) if result != golden["outcomes"][i]]
    assert not wrong, f"{len(wrong)} of {len(got)} cases differ from the record; the first: {wrong[:3]}"


def test_the_record_covers_what_it_is_meant_to():
    """The record itself: every outcome kind of the grid occurs, the unserved part reaches the engine errors of every keyword that has
    one, and the forwarding part saw both inner methods."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    of = lambda part: [golden["outcomes"][i] for i in golden[part]]
    grid = of("grid")
    assert "validated" in grid and {o[0] for o in grid if o != "validated"} == {"ValueError", "NotImplementedError"}
    assert {o[1] for o in grid if o != "validated"} == set(VALUES)
    unserved = {o[1] for o in of("unserved") if o != "validated" and o[2]}
    assert unserved == {"suffix_weights", "prefill", "sampler", "ddpm_sampler", "groups_attention", "batch_prefill"}
    forwarding = of("forwarding")
    assert "returned" not in grid + of("unserved") and any(o[1] == "returned" for o in forwarding)
    assert {call[0] for o in forwarding for call in o[0]} == {"predict_action_diff", "predict_action_diff_samples"}


def test_engine_key_with_every_mode_set():
    """The key suffix in its fixed order, every engine mode other than its default; the same modes again are the same engine."""
    from mla_amd import infer

    class Eng(infer._CachedEpsBase):
        def __init__(self, vlm, *ctor):
            self.ctor = ctor
    vlm = types.SimpleNamespace()
    every = dict(suffix_weights="fp8", prefill="compact", suffix_attention="split", prefill_precision="fp8", batch_prefill="fp8",
                 suffix_operand="once")
    eng = Eng._engine(vlm, "store", ("k", 1), ("first",), **every)
    assert list(vlm.store) == [("k", 1, "fp8", "prefill:compact", "attention:split", "precision:fp8", "batch_prefill:fp8", "operand:once")]
    assert Eng._engine(vlm, "store", ("k", 1), ("again",), **dict(reversed(list(every.items())))) is eng and eng.ctor == ("first",)
    assert Eng._engine(vlm, "store", ("k", 1), ("plain",)) is not eng and list(vlm.store)[1] == ("k", 1)


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"], "usage: PYTHONPATH=. python tests/test_sampling_modes_host.py --record (on the parent commit)"
    outcomes, record = [], {}
    for part in PARTS:
        record[part] = []
        for _, result in run(part):
            if result not in outcomes:
                outcomes.append(result)
            record[part].append(outcomes.index(result))
    record["outcomes"] = outcomes
    with open(GOLDEN, "w") as f:
        json.dump(record, f, separators=(",", ":"))
    print({part: len(record[part]) for part in record})
