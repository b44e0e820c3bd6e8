"""diffbindfr_amd -- MI355X-native reverse-diffusion sampler for DiffBindFR's pose-denoising
hot path (hand-written HIP for gfx950 behind the reference's registry boundary).

Importing the package registers ``TensorProductModelHIP`` (INTERACTION) and
``DiffBindFRHIP`` (MLDOCK_BUILDER); when the reference's ``druglib`` is importable they are
registered into its registries as well.
"""
from .registry import INTERACTION, MLDOCK_BUILDER, register_into_druglib  # noqa: F401
from .score_model import TensorProductModelHIP  # noqa: F401
from .sampler import DiffBindFRHIP  # noqa: F401
from . import vina  # noqa: F401
from . import modes  # noqa: F401
from . import posecheck  # noqa: F401
from . import trajectory  # noqa: F401
from . import sites  # noqa: F401
from . import interactions  # noqa: F401
from . import pocketcheck  # noqa: F401
from . import sasa  # noqa: F401
from . import apoholo  # noqa: F401
from . import hetero  # noqa: F401
from . import hydrogens  # noqa: F401
from . import decompose  # noqa: F401
from . import cavity  # noqa: F401
from . import pocketstates  # noqa: F401
from . import shapesim  # noqa: F401

register_into_druglib()
