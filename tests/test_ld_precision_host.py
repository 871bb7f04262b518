"""Host side of the opt-in f32 LD storage (no GPU): the command-line flag, the
VAMP argument's checks and the ctypes binding's two exports."""
import pytest

import hip_backend as hb
from main import build_parser
from sgvamp import VAMP


def test_cli_flag_default_and_choices(capsys):
    p = build_parser()
    assert p.parse_args([]).ld_precision == "f64"
    assert p.parse_args(["--ld-precision", "f32"]).ld_precision == "f32"
    assert p.parse_args(["--ld-precision", "f64"]).ld_precision == "f64"
    with pytest.raises(SystemExit):
        p.parse_args(["--ld-precision", "f16"])
    assert "f16" in capsys.readouterr().err
    text = p.format_help()
    assert "--ld-precision" in text and "f64" in text and "half" in text


def test_simulate_flag(monkeypatch):
    """simulate.py takes the same flag and hands it to simulate()."""
    import simulate

    seen = {}

    def fake(out, N, M, **kw):
        seen.update(kw)
        return {"ld": ["a"], "r": ["b"], "bim": ["c"], "beta": "d"}

    monkeypatch.setattr(simulate, "simulate", fake)
    simulate.main(["--out", "x", "--N", "10", "--M", "20", "--ld-precision", "f32"])
    assert seen["ld_precision"] == "f32"
    simulate.main(["--out", "x", "--N", "10", "--M", "20"])
    assert seen["ld_precision"] == "f64"
    with pytest.raises(SystemExit):
        simulate.main(["--out", "x", "--N", "10", "--M", "20", "--ld-precision", "bf16"])


def vamp(tmp_path, **kw):
    return VAMP(N=[100.0], Nt=100.0, M=10, K=1, rho=0.5, gamw=5.0, gam1=1e-6, a=[1.0],
                prior_vars=[0.0, 1.0], prior_probs=[0.99, 0.01], out_dir=str(tmp_path),
                out_name="t", write_files=False, **kw)


def test_vamp_ld_precision_argument(tmp_path):
    """Checked in the constructor, before any device call (no engine exists yet)."""
    assert vamp(tmp_path).ld_precision == "f64"
    v = vamp(tmp_path, ld_precision="f32")
    assert v.ld_precision == "f32" and v.engine is None
    with pytest.raises(ValueError, match="ld_packing"):
        vamp(tmp_path, ld_precision="f32", ld_packing=False)
    with pytest.raises(ValueError, match="ld_precision"):
        vamp(tmp_path, ld_precision="f16")
    assert vamp(tmp_path, ld_precision="f64", ld_packing=False).engine is None


def test_binding_exports():
    assert "sgv_set_ld_precision" in hb.EXPORTS
    assert "sgv_ld_block_precision" in hb.EXPORTS
