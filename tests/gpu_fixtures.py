"""Module-scoped fixtures the GPU tests import by name: the device and the score network with the seed-1 weights."""
import pytest
import torch

from tests.conv_hook import seeded_model


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return seeded_model(dev)
