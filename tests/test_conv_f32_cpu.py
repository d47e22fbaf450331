"""``iit_amd.ops.conv_f32`` and the ``--fp32-conv`` flag of ``train.py`` without a GPU: the default backend, what
``covered`` refuses (each with its counter) and the flag's exit when its requirements are missing."""
import pytest
import torch
from torch import nn

from iit_amd.entry import train
from iit_amd.ops import conv_f32


def _conv(cin=8, cout=8, k=3, channels_last=True, **kw):
    m = nn.Conv2d(cin, cout, k, padding=k // 2, bias=kw.pop("bias", False), **kw)
    return m.to(memory_format=torch.channels_last) if channels_last else m


def _x(n=2, c=8, h=6, w=6, dtype=torch.float32):
    return torch.randn(n, c, h, w, dtype=dtype).contiguous(memory_format=torch.channels_last)


def test_default_backend_is_torch():
    assert conv_f32.backend() == "torch"
    with pytest.raises(ValueError):
        conv_f32.set_backend("miopen")
    assert conv_f32.backend() == "torch"


@pytest.mark.parametrize("x, conv, counter", [
    (_x(), _conv(), "fallback_dtype"),  # a CPU tensor
    (_x(dtype=torch.bfloat16), _conv().to(torch.bfloat16), "fallback_dtype"),
    (_x(), _conv(channels_last=False), "fallback_layout"),  # an NCHW weight with k = 3
    (_x().contiguous(), _conv(), "fallback_layout"),  # an NCHW activation
    (_x(), _conv(bias=True), "fallback_geometry"),
    (_x(), _conv(groups=2), "fallback_geometry"),
    (_x(), _conv(dilation=2), "fallback_geometry"),
    (_x(), _conv(padding_mode="reflect"), "fallback_geometry"),
    (_x(), nn.Conv2d(8, 8, (3, 1), bias=False), "fallback_geometry"),
    (_x(), nn.Conv2d(8, 8, 3, stride=3, bias=False), "fallback_geometry"),
], ids=["cpu", "bf16", "nchw-weight", "nchw-activation", "bias", "groups", "dilation", "padding-mode", "non-square",
        "stride-3"])
def test_covered_refuses_and_counts(x, conv, counter):
    before = dict(conv_f32.calls)
    assert not conv_f32.covered(x, conv)
    delta = {n: v - before.get(n, 0) for n, v in conv_f32.calls.items() if v != before.get(n, 0)}
    assert delta == {counter: 1}


def test_layout_is_read_from_strides():
    # a 1 x 1 kernel's weight and a 1 x 1 activation are the same memory in both formats
    assert conv_f32.nhwc_dense(nn.Conv2d(8, 4, 1).weight) and conv_f32.nhwc_dense(torch.randn(3, 8, 1, 1))
    w3 = nn.Conv2d(8, 4, 3).weight
    assert w3.is_contiguous() and not conv_f32.nhwc_dense(w3)
    assert conv_f32.nhwc_dense(w3.detach().contiguous(memory_format=torch.channels_last))
    assert not conv_f32.nhwc_dense(_x()[:, :4])  # a channel slice is not dense
    assert conv_f32.geometry(_conv(k=7, stride=2)) == (7, 2, 3)


def test_train_flag_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        train.main(["--fp32-conv", "hip32", "--train-size", "8", "--test-size", "8", "--epochs", "1"])
    assert "--fp32-conv hip32 needs a GPU and --channels-last 1" in str(e.value)
    assert conv_f32.backend() == "torch"


def test_parse_defaults_are_unchanged():
    a = vars(train.parse([]))
    assert a.pop("fp32_conv") == "torch"
    assert a == {"task": "mnist_pvr", "train_size": 60000, "test_size": 10000, "batch_size": 256, "lr": 1e-3,
                 "epochs": 10, "mode": "q", "hook_point": "mod.layer3.mod.1.mod.conv2.hook_point", "wandb": False,
                 "save": None, "conv_benchmark": 0, "channels_last": 1}
    assert train.parse(["--fp32-conv", "hip32"]).fp32_conv == "hip32"
    with pytest.raises(SystemExit):
        train.parse(["--fp32-conv", "cudnn"])
