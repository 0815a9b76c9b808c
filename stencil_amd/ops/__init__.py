"""Native compute ops (hand-written gfx950 HIP kernels, csrc/src/*.hip),
re-exported at package level. Each op launches on a domain's compute
stream of the given ExchangeEngine; regions are global-coordinate Rect3s.

- jacobi_step: 7-point fp32 Jacobi with hot/cold sphere sources
  (csrc/src/jacobi.hip, z-marching float4 kernel)
- mhd_div_pass / mhd_substep: separable-derivative 6th-order MHD
  (csrc/src/mhd.hip)
- stencil_apply: generic weighted stencil described by a tap table
  (csrc/src/stencil_op.hip; StencilTaps / StencilType are its arguments)
- fill_f32 / init_harmonic_f64: field initialization (csrc/src/init.hip)
- field_stats: min/max/RMS reduction (csrc/src/reductions.hip)
- field_dot / field_axpby / cg_update: deterministic inner product,
  out = alpha x + beta y and the fused conjugate-gradient update on pitched
  quantities (csrc/src/vector_ops.hip); field_dot_begin / cg_update_begin
  + reduction_end split a reduction so that several local domains launch
  before any of them waits; field_scaled_update: out = alpha x + d (beta y +
  gamma z) with d a quantity
- field_sum / field_dot_sums / cg_update_sum / field_axpbyc: the sums that
  the projection off the constant null space needs, fused into the passes
  of field_dot, cg_update and field_axpby; their *_begin forms end with
  reduction_end_n
- field_axpby_norm2 / field_dot_pair / bicgstab_update: the three fused
  passes of a BiCGStab iteration (non-symmetric operators); their *_begin
  forms end with reduction_end / reduction_end_n
- diffusion_apply / diffusion_inv_diagonal: the variable-coefficient
  operator sigma I - div(k grad) and omega over its diagonal
  (csrc/src/diffusion_op.hip)
"""
from .._C import (  # noqa: F401
    FieldStats,
    MhdCoeffs,
    StencilTaps,
    StencilType,
    bicgstab_update,
    bicgstab_update_begin,
    cg_update,
    cg_update_begin,
    cg_update_sum,
    cg_update_sum_begin,
    diffusion_apply,
    diffusion_inv_diagonal,
    field_axpby,
    field_axpby_norm2,
    field_axpby_norm2_begin,
    field_axpbyc,
    field_dot,
    field_dot_begin,
    field_dot_pair,
    field_dot_pair_begin,
    field_dot_sums,
    field_dot_sums_begin,
    field_scaled_update,
    field_stats,
    field_sum,
    field_sum_begin,
    fill_f32,
    init_harmonic_f64,
    jacobi_step,
    mhd_div_pass,
    mhd_substep,
    reduction_end,
    reduction_end_n,
    stencil_apply,
)

# exactly the names imported above (nothing else here is public)
__all__ = [name for name in dir() if not name.startswith("_")]
