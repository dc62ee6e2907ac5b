"""The ResNet-18 state the inference tests share."""

import torch


def resnet_state(seed=3):
    """He-initialised parameters and a random BatchNorm state that makes the
    statistics matter: rm ~ N(0, 0.5), rv in [0.5, 2], gamma in [0.5, 1.5]."""
    from mpi_tensorflow_amd.models.generic import make_model

    model = make_model("resnet18")
    params = torch.zeros(model.layout.total)
    model.init_params(params, seed)
    g = torch.Generator().manual_seed(seed)
    views = model.layout.views(params)
    bn = {}
    for name, c in model.bn_channels.items():
        views[name + "_g"].copy_(torch.rand(c, generator=g) + 0.5)
        views[name + "_b"].copy_(torch.randn(c, generator=g) * 0.1)
        bn[name] = (torch.randn(c, generator=g) * 0.5, torch.rand(c, generator=g) * 1.5 + 0.5)
    return model, params, bn
