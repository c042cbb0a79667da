"""
The fully connected streamed engine's switch (mzx_net_set_fc_engine) on the serial test build: the config attribute, the
property round trip and the refusals.  The serial build accepts the setter and keeps running the per-operator program.
"""
import pytest
import torch

import hostcheck
from mzx import _lib, configs, models


@pytest.fixture(scope="module")
def be():
    return hostcheck.backend()


def test_config_attribute_property_round_trip_and_same_outputs(be):
    lib = be.lib
    torch.manual_seed(3)
    net = models.MuZeroNetwork(configs.cartpole(fc_dynamics_layers=[256, 256]), _backend=be)
    assert net.fc_engine == "ops" and lib.mzx_net_fc_engine(net.handle) == 0 and lib.mzx_net_fc_engine(None) == 0
    obs, act = torch.rand(5, 4), torch.arange(5) % 2
    before = net.recurrent_inference(net.initial_inference(obs)[3], act)
    net.fc_engine = "streamed"
    assert net.fc_engine == "streamed" and lib.mzx_net_fc_engine(net.handle) == 1
    for a, b in zip(before, net.recurrent_inference(net.initial_inference(obs)[3], act)):
        assert torch.equal(a, b)
    net.fc_engine = "ops"
    assert net.fc_engine == "ops"
    assert models.MuZeroNetwork(configs.cartpole(fc_engine="streamed"), _backend=be).fc_engine == "streamed"
    assert models.MuZeroNetwork(configs.cartpole(), _backend=be).fc_engine == "ops"


@pytest.mark.parametrize("overrides,text", [
    (dict(fc_value_layers=[1040]), "wider than 1024"),
    (dict(observation_shape=(1, 1, 4100)), "more than 4096"),
    (dict(fc_dynamics_layers=[1024], encoding_size=1024), "160 KiB"),
])
def test_refusals_by_name(be, overrides, text):
    net = models.MuZeroNetwork(configs.cartpole(**overrides), _backend=be)
    with pytest.raises(_lib.MzxError, match=text):
        net.fc_engine = "streamed"
    assert net.fc_engine == "ops"


def test_bad_values_and_residual_networks(be):
    lib = be.lib
    net = models.MuZeroNetwork(configs.cartpole(), _backend=be)
    for bad in (-1, 2):
        assert lib.mzx_net_set_fc_engine(net.handle, bad) == -1 and b"mzx_net_set_fc_engine" in lib.mzx_last_error()
    assert lib.mzx_net_set_fc_engine(None, 1) == -1
    with pytest.raises(ValueError):
        net.fc_engine = "mfma"
    resnet = models.MuZeroNetwork(configs.tictactoe(), _backend=be)
    with pytest.raises(_lib.MzxError, match="residual"):
        resnet.fc_engine = "streamed"
    with pytest.raises(_lib.MzxError, match="residual"):
        models.MuZeroNetwork(configs.tictactoe(fc_engine="streamed"), _backend=be)
