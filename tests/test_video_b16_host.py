"""CPU: the precision-mode surface of dcnet_amd/video.py that needs no GPU — the command line's --precision choices and the bank-size
arithmetic of VideoGrounder.bank_bytes_per_frame per mode."""
import pytest
import torch

from util import build_product, synth_sd


def test_command_line_precision_choices(capsys):
    from dcnet_amd import video as V
    assert sorted(V.BANK_BYTES_PER_VALUE) == ["bf16s", "fp32"]
    for bad in ("bf16", "fp8s", "fp16"):
        with pytest.raises(SystemExit):
            V.main(["--synthetic", "--precision", bad])
        assert "--precision" in capsys.readouterr().err


def test_bank_bytes_per_frame_by_mode(monkeypatch):
    from dcnet_amd import ops
    from dcnet_amd import video as V
    vg = V.VideoGrounder(build_product(256, synth_sd(256), torch.device("cpu")).eval(), n_frame=5)
    values = (8 * 8 + 16 * 16 + 32 * 32) * 512
    assert vg.bank_bytes_per_frame(256) == values * 8                      # fp32 rows + split
    assert vg.bank_bytes_per_frame(416) == (13 * 13 + 26 * 26 + 52 * 52) * 512 * 8
    monkeypatch.setattr(ops, "_precision", "bf16s")                        # (the mode's name only: nothing is launched)
    assert vg.bank_bytes_per_frame(256) == values * 6                      # bf16 rows + split or fp32 rows
    with pytest.raises(ValueError, match="size"):
        V.VideoGrounder(vg.model, n_frame=2).bank_bytes_per_frame()
    monkeypatch.setattr(ops, "_precision", "fp8s")
    with pytest.raises(RuntimeError, match="fp8s"):
        vg.bank_bytes_per_frame(256)
