"""diffdrr_amd: DiffDRR's rendering hot path on AMD Instinct MI355X (gfx950).

Drop-in for the Siddon ray-caster and trilinear ray-marcher of
eigenvivek/DiffDRR (``diffdrr/renderers.py``) as hand-written HIP kernels behind
the reference's own module API (``DRR``, ``Detector``, ``RigidTransform`` /
``convert``, ``Siddon``, ``Trilinear``, ``Registration``).  See DESIGN.md.
"""
__version__ = "0.1.0"

from .analytic import backproject, fbp_filter, fdk, ramp_taps  # noqa: F401
from .deformation import (  # noqa: F401
    FreeFormDeformation, JacobianStatistics, bspline_derivative_weights, bspline_weights, dense_field, field_jacobian,
    jacobian_determinant, jacobian_reference, jacobian_statistics, volume_penalty, volume_penalty_reference,
    warp_reference, warp_volume,
)
from .detector import Detector  # noqa: F401
from .drr import DRR  # noqa: F401
from .metrics import (  # noqa: F401
    GradientNormalizedCrossCorrelation2d,
    MultiscaleNormalizedCrossCorrelation2d,
    MutualInformation,
    NormalizedCrossCorrelation2d,
)
from .polyrigid import (  # noqa: F401
    PolyRigidDeformation,
    polyrigid_reference,
    polyrigid_warp,
    twist_lattice,
    weights_from_labels,
)
from .pose import RigidTransform, convert  # noqa: F401
from .reconstruction import (  # noqa: F401
    Fista,
    Reconstruction,
    TotalVariation3d,
    VolumeAdam,
    prox_total_variation_3d,
    total_variation_3d,
    tv_divergence_adjoint,
    tv_gradient_operator,
)
from .registration import (  # noqa: F401
    GraphedIteration, LevenbergMarquardt, MultiViewLevenbergMarquardt, PoseAdam, Registration,
    WeightedMultiViewLevenbergMarquardt,
)
from .renderers import Siddon, Trilinear  # noqa: F401
