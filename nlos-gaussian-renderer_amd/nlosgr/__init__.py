"""nlosgr — MI355X-native transient 3D-Gaussian NLOS renderer (hand-written HIP for gfx950).

Layers:
    nlosgr._lib            ctypes binding of the C ABI (include/nlosgr.h, libnlosgr.so)
    nlosgr.render          RenderFn: differentiable batched render (hist [P,T], optional per-ray)
    nlosgr.geometry        batched spherical sampling tables (spherical_sample_histogram for P walls)
    nlosgr.nlos_helpers    drop-in for the reference's nlos_helpers hot path (path T conventions)
    nlosgr.cuda_autograd   drop-in CUDARenderFunction / CUDARenderModule (path C conventions)
    nlosgr.rendering_cuda  drop-in GaussianRendererCUDA / create_cuda_renderer / CUDA_AVAILABLE
    nlosgr.volume          full transient-volume render + MSE loss (the benchmarked step)
    nlosgr.distributed     relay-wall sharding over ranks + one all-reduce of Gaussian gradients
    nlosgr.train           fused training iteration (nlosgr_mse + render fwd/bwd + nlosgr_adam)
    nlosgr.data            Zaragoza capture format, data_shuffle, whole-volume targets / geometry
    nlosgr.checkpoint      reference-keyed checkpoints loadable with weights_only=True
    nlosgr.voxelize        reconstruction output: Gaussians -> voxel grid, max projections, depth map
    nlosgr.mesh            surface output: isosurface of a voxelized field as a triangle mesh, PLY export
    nlosgr.backproject     the capture on a voxel grid: back-projection, time filters, backproject_capture
    nlosgr.phasor          phasor-field reconstruction: complex back-projection in one pass, phasor_capture
    nlosgr.fk              f-k migration of a confocal capture: three HIP passes around torch.fft, fk_capture
    nlosgr.rsd             fast phasor field (Rayleigh-Sommerfeld diffraction by FFT on the wall's lattice): four HIP
                           passes around torch.fft, rsd_capture; confocal or one laser spot
    nlosgr.lct             light-cone transform of a confocal capture (Wiener-filtered inversion): four HIP passes
                           around torch.fft, lct_capture; LctOperator, the confocal forward operator and its adjoint
                           at FFT speed, lct_solve (Landweber, FISTA), lct_solve_pd (TV, sparsity, a Poisson data
                           term), lct_solve_capture
    nlosgr.prox            the primal-dual solver behind lct_solve_pd: three HIP passes (the row prox, the TV dual
                           and primal updates) and the loop over two operator callables, primal_dual
    nlosgr.lattice         the wall's lattice that fk, rsd and lct share: wall_lattice, the row lookup, the capture
                           prologue and crop
    nlosgr.forward_project its adjoint: voxel grid -> transients, voxel_transient, operator_norm, landweber
                           (both take lasers= for a non-confocal capture: the laser spot differs from the sensed one)
    nlosgr.irf             temporal instrument response: IRF, gaussian_irf, convolve_time (render -> capture)
    nlosgr.loss            photon-count likelihood: fused loss(kind=), PoissonDeviance, simulate_capture
"""
from . import _lib  # noqa: F401
from .geometry import Geometry, build_geometry, relay_wall_grid, volume_box_point  # noqa: F401
from .model import GaussianParams, features_flat  # noqa: F401
from .render import RenderConfig, RenderFn, bboxes, render, render_backward, render_forward  # noqa: F401

__all__ = ["Geometry", "build_geometry", "relay_wall_grid", "volume_box_point", "GaussianParams",
           "features_flat", "RenderConfig", "RenderFn", "render", "render_forward", "render_backward", "bboxes",
           "Mesh", "isosurface", "extract_mesh", "write_ply", "read_ply",
           "backproject_capture", "time_filter", "phasor_capture", "phasor_kernel",
           "fk_capture", "fk_migrate", "rsd_capture", "rsd_reconstruct", "lct_capture", "lct_reconstruct",
           "LctOperator", "lct_project", "lct_adjoint", "lct_solve", "lct_solve_capture", "lct_load_volume",
           "lct_store_rows", "lct_load_rows", "lct_store_volume", "lct_solve_pd",
           "primal_dual", "prox_rows", "tv_dual_step", "tv_primal_step", "tv_gradient", "tv_divergence"]

_BP_NAMES = ("backproject_capture", "time_filter")
_PH_NAMES = ("phasor_capture", "phasor_kernel")
_FK_NAMES = ("fk_capture", "fk_migrate")
_RSD_NAMES = ("rsd_capture", "rsd_reconstruct")
_LCT_NAMES = ("lct_capture", "lct_reconstruct", "LctOperator", "lct_project", "lct_adjoint", "lct_solve",
              "lct_solve_capture", "lct_load_volume", "lct_store_rows", "lct_load_rows", "lct_store_volume",
              "lct_solve_pd")
_PROX_NAMES = ("primal_dual", "prox_rows", "tv_dual_step", "tv_primal_step", "tv_gradient", "tv_divergence")
_MESH_NAMES = ("Mesh", "isosurface", "extract_mesh", "write_ply", "read_ply")


def __getattr__(name):
    # nlosgr.mesh is imported on first use, so `python -m nlosgr.mesh` runs it as __main__ only
    if name in _MESH_NAMES:
        from . import mesh
        return getattr(mesh, name)
    # the same for `python -m nlosgr.backproject` (nlosgr.backproject itself is the module; its function of the
    # same name is nlosgr.backproject.backproject)
    if name in _BP_NAMES:
        from . import backproject
        return getattr(backproject, name)
    if name in _PH_NAMES:
        from . import phasor
        return getattr(phasor, name)
    if name in _FK_NAMES:
        from . import fk
        return getattr(fk, name)
    if name in _RSD_NAMES:
        from . import rsd
        return getattr(rsd, name)
    if name in _LCT_NAMES:
        from . import lct
        return getattr(lct, name)
    if name in _PROX_NAMES:
        from . import prox
        return getattr(prox, name)
    raise AttributeError(f"module 'nlosgr' has no attribute {name!r}")
