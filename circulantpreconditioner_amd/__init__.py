"""MI355X-native circulant / block-circulant FFT preconditioner.

The product is ``lib/libcirculant_fft.so`` (hand-written HIP kernels for gfx950 +
a C ABI, ``include/*.h``).  This package is the Python host mirror of the
reference's operator interface (``src/FftLinearSolver_3D.h``,
``src/PCSHELLFft_3D.hxx``); PyTorch supplies device memory and streams only.
"""
from ._lib import CirculantError, LIB_PATH, lib  # noqa: F401
from .plan import (CirculantPlan, RealPlan, advdiff_symbol_1d, advdiff_z_ratio, build_diag_3d,  # noqa: F401
                   fill_uniform, mixed_pass_class, pointwise_divide, scale, transport_symbol_1d, upwind_to_advdiff,
                   z_route)

__version__ = "0.1.0"
