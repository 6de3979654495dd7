"""The command lines of the six latent-pipeline scripts did not move: each script's argparse action table, rebuilt from its
`build_parser()`, equals tests/golden/latent_cli_options_v1.json, which was dumped from the scripts as they were before their shared
options moved into s2p_amd/latent_cli.py (train_cql's with its extension of train_iql's parser applied).  No device is needed."""
import json
import os

import pytest

SCRIPTS = ("train_latent", "train_iql", "train_cql", "evaluate_policy", "predict_latent", "imagine_policy")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_cli_options_v1.json")


def option_table(parser):
    """One row per action, in the parser's order."""
    return [dict(option_strings=list(a.option_strings), dest=a.dest, default=a.default, type=a.type.__name__ if a.type else None,
                 choices=list(a.choices) if a.choices is not None else None, required=a.required, nargs=a.nargs, help=a.help)
            for a in parser._actions]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_the_six_scripts(golden):
    assert sorted(golden) == sorted(SCRIPTS) and all(len(rows) > 5 for rows in golden.values())
    assert [r["dest"] for r in golden["train_cql"]][:len(golden["train_iql"])] == [r["dest"] for r in golden["train_iql"]]


@pytest.mark.parametrize("script", SCRIPTS)
def test_option_table_is_the_recorded_one(script, golden):
    got = json.loads(json.dumps(option_table(__import__(script).build_parser())))
    want = golden[script]
    assert [r["dest"] for r in got] == [r["dest"] for r in want]                       # the order too
    for g, w in zip(got, want):
        assert g == w, (script, w["dest"])


def test_chain_form_is_one_of_four_and_reads_chain_compute_only_for_a_fused_no_grad_chain():
    import itertools
    import types

    from s2p_amd.slac import LatentModel
    for fused, grad, compute, keep in itertools.product((False, True), (False, True), ("fp32", "bf16", "fp16"), (False, True)):
        m = types.SimpleNamespace(fused_chain=fused, fused_chain_grad=grad, chain_compute=compute)
        if keep:
            want = "fused_save" if grad else "layers"
        elif not fused:
            want = "layers"
        elif compute == "fp16":
            with pytest.raises(ValueError, match="chain_compute is 'fp32' or 'bf16', not 'fp16'"):
                LatentModel.chain_form(m, keep)
            continue
        else:
            want = "fused_bf16" if compute == "bf16" else "fused"
        assert LatentModel.chain_form(m, keep) == want, (fused, grad, compute, keep)


def test_chain_settings_follow_the_options_a_script_has():
    import imagine_policy
    import train_iql
    import train_latent
    from s2p_amd.latent_cli import chain_settings
    base = ["--real", "r.npz", "--steps", "1", "--out", "o"]
    assert chain_settings(train_latent.parse_args(base + ["--fused_chain_grad"])) == dict(fused_chain=False, fused_chain_grad=True,
                                                                                          chain_compute="fp32")
    a = train_iql.parse_args(base + ["--latent_dir", "d", "--fused_chain", "--bf16_chain"])
    assert chain_settings(a) == dict(fused_chain=True, fused_chain_grad=False, chain_compute="bf16")
    a = imagine_policy.parse_args(["--data", "d.npz", "--latent_dir", "d", "--policy_dir", "p", "--out", "o.npz", "--fused_chain"])
    assert chain_settings(a) == dict(fused_chain=True, fused_chain_grad=False, chain_compute="fp32") and not hasattr(a, "bf16_chain")


def test_one_parser_per_call():
    import train_cql
    import train_iql
    a, b = train_iql.build_parser(), train_iql.build_parser()
    assert a is not b and "--num_random" not in a._option_string_actions               # train_cql's extension does not leak
    assert "--num_random" in train_cql.build_parser()._option_string_actions
    assert train_cql.build_parser().description == train_cql.__doc__ and a.description == train_iql.__doc__
