"""Linear solvers on top of the stencil operator and the vector operations
of DistributedDomain (dot, axpby, cg_update)."""
from .cg import CGResult, ConjugateGradient

__all__ = ["CGResult", "ConjugateGradient"]
