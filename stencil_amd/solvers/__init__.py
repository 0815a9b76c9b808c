"""Linear solvers on top of the stencil operator and the vector operations
of DistributedDomain (dot, axpby, axpbypcz, cg_update), and the geometric
multigrid preconditioner with its grid transfer."""
from .cg import CGResult, ConjugateGradient
from .multigrid import GeometricMultigrid
from .transfer import GridTransfer

__all__ = ["CGResult", "ConjugateGradient", "GeometricMultigrid", "GridTransfer"]
