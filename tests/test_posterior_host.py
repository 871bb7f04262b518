"""Host side of the opt-in posterior outputs (no GPU): the command-line flags,
the VAMP arguments' checks, and the binding against the header."""
import os
import re

import pytest

import hip_backend as hb
from main import build_parser
from sgvamp import VAMP
from tests.conftest import ROOT


def test_cli_flags_defaults_and_choices(capsys):
    p = build_parser()
    a = p.parse_args([])
    assert a.posterior == "none" and a.pip_threshold == 0.95
    for mode in ("none", "last", "all"):
        assert p.parse_args(["--posterior", mode]).posterior == mode
    assert p.parse_args(["--pip-threshold", "0.5"]).pip_threshold == 0.5
    assert p.parse_args(["--pip-threshold", "1"]).pip_threshold == 1.0
    with pytest.raises(SystemExit):
        p.parse_args(["--posterior", "first"])
    assert "first" in capsys.readouterr().err
    text = p.format_help()
    assert "--posterior" in text and "--pip-threshold" in text
    assert "lodds" in text and "damped" in text


@pytest.mark.parametrize("bad", ["1.5", "-0.1", "nan", "often"])
def test_bad_pip_threshold_is_refused_with_a_message(bad, capsys):
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--pip-threshold=" + bad])
    err = capsys.readouterr().err
    assert "--pip-threshold" in err and "probability in [0, 1]" in err and bad in err


def vamp(tmp_path, **kw):
    return VAMP(N=[100.0], Nt=100.0, M=10, K=1, rho=0.5, gamw=5.0, gam1=1e-6, a=[1.0],
                prior_vars=[0.0, 1.0], prior_probs=[0.99, 0.01], out_dir=str(tmp_path),
                out_name="t", **kw)


def test_vamp_posterior_arguments(tmp_path):
    """Checked in the constructor, before any device call; the CSV header is
    written only when the feature is on."""
    v = vamp(tmp_path)
    assert v.posterior_mode is None and v.pip_threshold == 0.95 and v.engine is None
    assert sorted(os.listdir(tmp_path)) == ["t_cohort_1.csv", "t_metrics.csv"]
    with pytest.raises(ValueError, match="posterior"):
        vamp(tmp_path, posterior="first")
    with pytest.raises(ValueError, match="posterior"):
        vamp(tmp_path, posterior="none")
    for bad in (1.5, -0.1, float("nan"), "often"):
        with pytest.raises(ValueError, match="pip_threshold"):
            vamp(tmp_path, posterior="all", pip_threshold=bad)
    v = vamp(tmp_path, posterior="last", pip_threshold=0.5)
    assert v.posterior_mode == "last" and v.pip_threshold == 0.5 and v.engine is None
    assert open(tmp_path / "t_posterior.csv").read() == "it\tsum_pip\tsum_postvar\tn_pip_ge_thr\n"
    with pytest.raises(ValueError, match="iteration count"):
        v.begin(iterations=None)
    assert "damped" in VAMP.__doc__ and "damped" in VAMP.posterior.__doc__


def test_binding_follows_the_header():
    text = open(os.path.join(ROOT, "include", "sgvamp_hip.h")).read()
    m = re.search(r"^#define SGV_STEP_POSTERIOR\s+(\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == hb.STEP_POSTERIOR == 256
    for n in ("EM", "DENOISE_DAMP", "ALPHA1_DAMP", "LMMSE_DAMP", "LEARN_GAMW", "METRICS", "CHAIN",
              "MLE"):
        assert not getattr(hb, "STEP_" + n) & hb.STEP_POSTERIOR
    assert "sgv_posterior" in hb.EXPORTS and "sgv_set_posterior_outputs" in hb.EXPORTS
    assert len(hb._SIGS["sgv_posterior"]) == 13      # ctx + the header's 12 parameters
    assert hb.ABI_VERSION == 2
    lib = hb.load()
    assert hasattr(lib, "sgv_posterior") and hasattr(lib, "sgv_set_posterior_outputs")
