"""Linear solvers on top of the stencil operator and the vector operations
of DistributedDomain (dot, axpby, axpbypcz, scaled_update, cg_update), the
variable-coefficient diffusion operator with its Jacobi preconditioner,
the geometric multigrid preconditioner with its grid transfer, and BiCGStab
for non-symmetric stencils (axpby_norm2, dot_pair, bicgstab_update). The
argument checks and the operator application they share are in _common.py."""
from .bicgstab import BiCGStab
from .cg import CGResult, ConjugateGradient
from .diffusion import DiffusionOperator, JacobiPreconditioner
from .multigrid import GeometricMultigrid
from .transfer import GridTransfer

__all__ = ["BiCGStab", "CGResult", "ConjugateGradient", "DiffusionOperator",
           "GeometricMultigrid", "GridTransfer", "JacobiPreconditioner"]
