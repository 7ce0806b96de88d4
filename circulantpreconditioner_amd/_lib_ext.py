"""The ctypes layer of both libraries: the structs and the one signature table.

``libcirculant_fft.so`` (PetscScalar = complex) and ``libcirculant_fft_real.so`` (PetscScalar =
double) export the same C functions; ``signatures(S)`` is the one table of them, a function of
the scalar type S (``PetscScalar`` or ``ctypes.c_double``), grouped by the header that declares
them and tagged with the build that holds each group.  ``declare`` loads it strictly: a name the
table promises and the library lacks raises.  To bind a new C function for both builds, add one
line to its header's group here (and a method to the class in ``_boundary.py`` that wraps it).
"""
from __future__ import annotations

import ctypes
import functools
import types

BOTH, COMPLEX_BUILD, REAL_BUILD = "both", "complex", "real"  # which build holds a group of the table


class PetscScalar(ctypes.Structure):
    """PetscScalar of a complex PETSc build (std::complex<double> / double _Complex)."""
    _fields_ = [("re", ctypes.c_double), ("im", ctypes.c_double)]

    @classmethod
    def of(cls, v) -> "PetscScalar":
        c = complex(v)
        return cls(c.real, c.imag)

    def __complex__(self):
        return complex(self.re, self.im)


@functools.lru_cache(maxsize=None)
def context_structs(S) -> types.SimpleNamespace:
    """The four context structs that hold PetscScalar members, for S = PetscScalar or c_double
    (built once per scalar type).

    FFTPrecTransportContext: the reference's exact 12 members (src/PCSHELLFft_3D.hxx:8-21); this
    build's additions live in a side table (FFTPrecTransportContextSetRemapBack) and the plan
    behind FFT_MAT.  FFTPrecDiffusionContext (include/diffusion_equation.h): those 12 members in
    order, then mu_x, mu_y, mu_z.  StructuredTransportContext (src/FftLinearSolver_3D.h:7-19) and
    StructuredDiffusionContext (include/diffusion_equation.h) are passed by value."""
    i64, vp = ctypes.c_int64, ctypes.c_void_p

    def struct(name, fields):
        return type(name, (ctypes.Structure,), {"_fields_": fields})

    transport = ([("spaceDim", i64), ("n_x", i64), ("n_y", i64), ("n_z", i64)]
                 + [(k, S) for k in ("lambda_x", "lambda_y", "lambda_z")]
                 + [(k, vp) for k in ("FFT_MAT", "intersectionMatrix", "Diag", "b_hat", "b_cartesien")])
    grid = [("n_x", i64), ("n_y", i64), ("n_z", i64)]
    spacing = [(k, S) for k in ("dt", "delta_x", "delta_y", "delta_z")] + [("FFT_MAT", vp)]
    return types.SimpleNamespace(
        FFTPrecTransportContext=struct("FFTPrecTransportContext", transport),
        FFTPrecDiffusionContext=struct("FFTPrecDiffusionContext",
                                       transport + [(k, S) for k in ("mu_x", "mu_y", "mu_z")]),
        StructuredTransportContext=struct("StructuredTransportContext",
                                          grid + [(k, S) for k in ("a_x", "a_y", "a_z")] + spacing),
        StructuredDiffusionContext=struct("StructuredDiffusionContext",
                                          grid + [(k, S) for k in ("a_x", "a_y", "a_z", "nu")] + spacing))


# the complex build's structs under their own names
_C = context_structs(PetscScalar)
FFTPrecTransportContext, FFTPrecDiffusionContext = _C.FFTPrecTransportContext, _C.FFTPrecDiffusionContext
StructuredTransportContext, StructuredDiffusionContext = _C.StructuredTransportContext, _C.StructuredDiffusionContext


class _ResultDict:
    """as_dict() of a time loop's result struct: the members by name, an array member as a list
    under its name less the trailing underscore, dev_ms / dev_launches keyed by kernel class."""

    def as_dict(self) -> dict:
        d = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            if k in ("dev_ms_", "dev_launches_"):
                d[k[:-1]] = dict(zip(("pcapply", "matmult", "vector", "copy"), v))
            elif issubclass(t, ctypes.Array):
                d[k.rstrip("_")] = list(v)
            else:
                d[k] = v
        return d


class TransportConfig(ctypes.Structure):
    """cfp_transport_config (include/transport_equation.h)."""
    _fields_ = [("nx", ctypes.c_int64), ("ny", ctypes.c_int64), ("nz", ctypes.c_int64),
                ("xmin", ctypes.c_double * 3), ("xmax", ctypes.c_double * 3), ("a", ctypes.c_double * 3),
                ("cfl", ctypes.c_double), ("tmax", ctypes.c_double), ("ntmax", ctypes.c_int64),
                ("precision", ctypes.c_double), ("max_its", ctypes.c_int64), ("restart", ctypes.c_int64),
                ("pc", ctypes.c_int), ("sign_mode", ctypes.c_int), ("lambda_mode", ctypes.c_int),
                ("pc_side", ctypes.c_int), ("on_device", ctypes.c_int), ("fuse", ctypes.c_int),
                ("profile", ctypes.c_int)]


class TransportResult(_ResultDict, ctypes.Structure):
    """cfp_transport_result (include/transport_equation.h)."""
    _fields_ = [("steps", ctypes.c_int64), ("dt", ctypes.c_double), ("time", ctypes.c_double),
                ("total_its", ctypes.c_int64), ("max_step_its", ctypes.c_int64), ("min_step_its", ctypes.c_int64),
                ("last_reason", ctypes.c_int), ("all_converged", ctypes.c_int), ("last_residual", ctypes.c_double),
                ("last_norm_dU", ctypes.c_double), ("solve_seconds", ctypes.c_double),
                ("pc_seconds", ctypes.c_double), ("pc_calls", ctypes.c_int64), ("setup_seconds", ctypes.c_double),
                ("lambda_", ctypes.c_double * 3), ("loop_seconds", ctypes.c_double), ("dev_ms_", ctypes.c_double * 4),
                ("dev_launches_", ctypes.c_int64 * 4), ("fused_dots", ctypes.c_int64), ("fused_norms", ctypes.c_int64),
                ("rstart", ctypes.c_int64), ("nlocal", ctypes.c_int64)]


class AdvDiffConfig(ctypes.Structure):
    """cfp_advdiff_config (include/diffusion_equation.h)."""
    _fields_ = [("nx", ctypes.c_int64), ("ny", ctypes.c_int64), ("nz", ctypes.c_int64),
                ("xmin", ctypes.c_double * 3), ("xmax", ctypes.c_double * 3), ("a", ctypes.c_double * 3),
                ("nu", ctypes.c_double), ("dt", ctypes.c_double), ("tmax", ctypes.c_double), ("ntmax", ctypes.c_int64),
                ("precision", ctypes.c_double), ("max_its", ctypes.c_int64), ("restart", ctypes.c_int64),
                ("pc", ctypes.c_int), ("bc", ctypes.c_int), ("pc_side", ctypes.c_int), ("on_device", ctypes.c_int),
                ("profile", ctypes.c_int)]


class AdvDiffResult(_ResultDict, ctypes.Structure):
    """cfp_advdiff_result (include/diffusion_equation.h)."""
    _fields_ = [("steps", ctypes.c_int64), ("dt", ctypes.c_double), ("time", ctypes.c_double),
                ("total_its", ctypes.c_int64), ("max_step_its", ctypes.c_int64), ("min_step_its", ctypes.c_int64),
                ("last_reason", ctypes.c_int), ("all_converged", ctypes.c_int), ("last_residual", ctypes.c_double),
                ("last_norm_dU", ctypes.c_double), ("solve_seconds", ctypes.c_double),
                ("pc_seconds", ctypes.c_double), ("pc_calls", ctypes.c_int64), ("setup_seconds", ctypes.c_double),
                ("lambda_", ctypes.c_double * 3), ("mu_", ctypes.c_double * 3), ("loop_seconds", ctypes.c_double),
                ("dev_ms_", ctypes.c_double * 4), ("dev_launches_", ctypes.c_int64 * 4),
                ("fused_dots", ctypes.c_int64), ("fused_norms", ctypes.c_int64),
                ("rstart", ctypes.c_int64), ("nlocal", ctypes.c_int64)]


class AIJInfo(ctypes.Structure):
    """PetscMiniAIJInfo (include/petsc_mini.h): the device form an AIJ's MatMult will use."""
    _fields_ = [("format", ctypes.c_int), ("B", ctypes.c_int), ("nd", ctypes.c_int), ("ncls", ctypes.c_int),
                ("nblk", ctypes.c_int), ("re", ctypes.c_int), ("lds_bytes", ctypes.c_int64)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_}
        d["format"] = {0: "csr", 1: "dia", 2: "bdia"}[d["format"]]
        return d


class WaveConfig(ctypes.Structure):
    """cfp_wave_config (include/wave_system.h)."""
    _fields_ = [("nx", ctypes.c_int64), ("ny", ctypes.c_int64), ("nz", ctypes.c_int64),
                ("xmin", ctypes.c_double * 3), ("xmax", ctypes.c_double * 3), ("c0", ctypes.c_double),
                ("cfl", ctypes.c_double), ("tmax", ctypes.c_double), ("ntmax", ctypes.c_int64),
                ("precision", ctypes.c_double), ("max_its", ctypes.c_int64), ("restart", ctypes.c_int64),
                ("pc", ctypes.c_int), ("bc", ctypes.c_int), ("pc_side", ctypes.c_int), ("on_device", ctypes.c_int),
                ("dim", ctypes.c_int), ("profile", ctypes.c_int), ("fuse", ctypes.c_int)]


class WaveResult(_ResultDict, ctypes.Structure):
    """cfp_wave_result (include/wave_system.h)."""
    _fields_ = [("steps", ctypes.c_int64), ("dt", ctypes.c_double), ("time", ctypes.c_double),
                ("total_its", ctypes.c_int64), ("max_step_its", ctypes.c_int64), ("min_step_its", ctypes.c_int64),
                ("last_reason", ctypes.c_int), ("all_converged", ctypes.c_int), ("last_residual", ctypes.c_double),
                ("last_norm_dU", ctypes.c_double), ("solve_seconds", ctypes.c_double),
                ("pc_seconds", ctypes.c_double), ("pc_calls", ctypes.c_int64), ("setup_seconds", ctypes.c_double),
                ("kappa", ctypes.c_double * 3), ("rstart", ctypes.c_int64), ("nlocal", ctypes.c_int64),
                ("loop_seconds", ctypes.c_double), ("dev_ms_", ctypes.c_double * 4),
                ("dev_launches_", ctypes.c_int64 * 4), ("fused_dots", ctypes.c_int64), ("fused_norms", ctypes.c_int64)]


class FFTPrecWaveContext(ctypes.Structure):
    """struct FFTPrecWaveContext (include/wave_system.h)."""
    _fields_ = [("n_x", ctypes.c_int64), ("n_y", ctypes.c_int64), ("n_z", ctypes.c_int64),
                ("kappa_x", ctypes.c_double), ("kappa_y", ctypes.c_double), ("kappa_z", ctypes.c_double),
                ("c0", ctypes.c_double), ("plan", ctypes.c_void_p), ("dim", ctypes.c_int64)]


class FFTPrecWaveRealContext(ctypes.Structure):
    """struct FFTPrecWaveRealContext (include/wave_system_real.h): FFTPrecWaveContext's members and
    order, `plan` a cfp_wave_rplan_t; the same struct in both scalar builds (no PetscScalar member)."""
    _fields_ = list(FFTPrecWaveContext._fields_)


def signatures(S) -> list:
    """The signature table: [(group, build, {name: (argtypes, restype)})].  S is PetscScalar (by
    value a 16-byte struct) or c_double; a group is the header that declares its functions, and
    `build` says which library holds them: BOTH, COMPLEX_BUILD (the transport, wave and mesh drivers,
    whose sources the real-scalar library does not compile) or REAL_BUILD."""
    i64, u64, c_int, d, cs = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
    vp = dp = ctypes.c_void_p  # a handle / a device pointer
    P, C = ctypes.POINTER, context_structs(S)
    return [
        ("circulant_fft.h", BOTH, {
            "cfp_version": ([], cs),
            "cfp_last_error": ([], cs),
            "cfp_device_count": ([P(c_int)], c_int),
            "cfp_stream_sync": ([vp], c_int),
            "cfp_device_copy": ([vp, vp, ctypes.c_size_t, vp], c_int),
            "cfp_plan_create": ([P(vp), i64, i64, i64, c_int], c_int),
            "cfp_plan_destroy": ([vp], c_int),
            "cfp_plan_set_symbol_transport": ([vp, dp], c_int),
            "cfp_plan_set_symbol_separable": ([vp, dp, dp, dp, dp], c_int),
            "cfp_plan_set_diag": ([vp, dp, c_int], c_int),
            "cfp_plan_get_diag": ([vp, dp, vp], c_int),
            "cfp_plan_symbol_version": ([vp, P(u64)], c_int),
            "cfp_plan_apply": ([vp, dp, dp, vp], c_int),
            "cfp_plan_apply_ex": ([vp, dp, dp, vp, vp], c_int),
            "cfp_plan_apply_with_diag": ([vp, dp, dp, dp, vp], c_int),
            "cfp_plan_apply_host": ([vp, dp, dp], c_int),
            "cfp_plan_apply_with_diag_host": ([vp, dp, dp, dp], c_int),
            "cfp_plan_forward": ([vp, dp, dp, vp], c_int),
            "cfp_plan_backward": ([vp, dp, dp, vp], c_int),
            "cfp_plan_set_chunking": ([vp, i64], c_int),
            "cfp_plan_set_graph": ([vp, c_int], c_int),
            "cfp_plan_set_schedule": ([vp, c_int], c_int),
            "cfp_plan_set_three_pass_shape": ([vp, c_int, c_int], c_int),
            "cfp_plan_num_passes": ([vp, P(c_int)], c_int),
            "cfp_plan_pass_info": ([vp, c_int, P(c_int), P(c_int), P(i64), P(c_int), P(c_int)], c_int),
            "cfp_plan_time_passes": ([vp, dp, dp, c_int, dp, vp], c_int),
            "cfp_plan_profile_begin": ([vp, c_int, c_int], c_int),
            "cfp_plan_profile_end": ([vp, dp, P(c_int)], c_int),
            "cfp_pointwise_divide": ([dp, dp, dp, i64, vp], c_int),
            "cfp_scale": ([dp, d, d, i64, vp], c_int),
            "cfp_fill_uniform": ([dp, i64, u64, i64, vp], c_int),
            "cfp_build_diag_3d": ([dp, dp, dp, dp, i64, i64, i64, dp, vp], c_int),
            "cfp_transport_symbol_1d": ([i64, dp], c_int),
            "cfp_plan_mid_kernel": ([vp, P(c_int)], c_int),
            "cfp_transport_z_ratio": ([i64, i64, dp, P(d)], c_int),
            "cfp_plan_set_symbol_advdiff": ([vp, dp, dp], c_int),
            "cfp_plan_set_symbol_upwind": ([vp, dp, dp], c_int),
            "cfp_upwind_to_advdiff": ([dp, dp, dp, dp], c_int),
            "cfp_advdiff_symbol_1d": ([i64, P(d), P(d), dp], c_int),
            "cfp_advdiff_z_ratio": ([i64, i64, dp, dp, P(d)], c_int),
            "cfp_symbol_z_route": ([i64, i64, i64, dp, dp, c_int, P(c_int), P(d)], c_int),
            "cfp_mixed_pass_class": ([c_int, i64, c_int, c_int, P(c_int), P(c_int), P(c_int), P(c_int), P(i64),
                                      P(c_int), P(c_int)], c_int),
        }),
        ("circulant_fft_real.h", BOTH, {
            "cfp_rplan_create": ([P(vp), i64, i64, i64, c_int], c_int),
            "cfp_rplan_destroy": ([vp], c_int),
            "cfp_rplan_set_symbol_transport": ([vp, P(d)], c_int),
            "cfp_rplan_set_symbol_advdiff": ([vp, P(d), P(d)], c_int),
            "cfp_rplan_set_symbol_upwind": ([vp, P(d), P(d)], c_int),
            "cfp_rplan_set_mid_kernel": ([vp, c_int], c_int),
            "cfp_rplan_mid_kernel": ([vp, P(c_int)], c_int),
            "cfp_rplan_apply": ([vp, vp, vp, vp], c_int),
            "cfp_rplan_num_passes": ([vp, P(c_int)], c_int),
            "cfp_rplan_time_passes": ([vp, vp, vp, c_int, P(d), vp], c_int),
            "cfp_rplan_set_schedule": ([vp, c_int], c_int),
            "cfp_rplan_schedule": ([vp, P(c_int)], c_int),
        }),
        # slab-distributed plan over RCCL + single-process group
        ("circulant_fft_dist.h", BOTH, {
            "cfp_dist_get_unique_id": ([cs], c_int),
            "cfp_dist_unique_id_bytes": ([], c_int),
            "cfp_slab_layout": ([i64, i64, i64, c_int, c_int, P(i64)], c_int),
            "cfp_slab_work_size": ([i64, i64, i64, c_int, c_int, P(i64)], c_int),
            "cfp_slab_num_steps": ([i64, i64, i64, c_int, c_int, P(c_int)], c_int),
            "cfp_slab_step_info": ([i64, i64, i64, c_int, c_int, c_int, P(i64), P(d)], c_int),
            "cfp_dist_plan_create": ([P(vp), i64, i64, i64, c_int, c_int, cs, c_int], c_int),
            "cfp_dist_plan_create_timeout": ([P(vp), i64, i64, i64, c_int, c_int, cs, c_int, d], c_int),
            "cfp_dist_plan_rccl_info": ([vp, P(c_int), P(c_int), P(c_int), P(d), cs, c_int], c_int),
            "cfp_rccl_version": ([P(c_int), cs, c_int], c_int),
            "cfp_rccl_blocking": ([P(c_int)], c_int),
            "cfp_dist_plan_destroy": ([vp], c_int),
            "cfp_dist_plan_create_external": ([P(vp), i64, i64, i64, c_int, c_int, c_int], c_int),
            "cfp_dist_plan_work_buffer": ([vp, P(vp)], c_int),
            "cfp_dist_plan_run_segment": ([vp, c_int, dp, dp, vp], c_int),
            "cfp_dist_plan_set_work_buffer": ([vp, dp], c_int),
            "cfp_dist_plan_set_symbol_transport": ([vp, dp], c_int),
            "cfp_dist_plan_apply": ([vp, dp, dp, vp], c_int),
            "cfp_dist_plan_profile_begin": ([vp, c_int, c_int], c_int),
            "cfp_dist_plan_profile_end": ([vp, dp, P(c_int)], c_int),
            "cfp_dist_plan_local_size": ([vp, P(i64)], c_int),
            "cfp_dist_plan_time_phases": ([vp, dp, dp, c_int, dp, vp], c_int),
            "cfp_dist_plan_num_phases": ([vp, P(c_int)], c_int),
            "cfp_dist_plan_phase_info": ([vp, c_int, P(c_int), P(c_int), P(c_int), P(c_int)], c_int),
            "cfp_group_create": ([P(vp), i64, i64, i64, c_int, P(c_int)], c_int),
            "cfp_group_destroy": ([vp], c_int),
            "cfp_group_set_symbol_transport": ([vp, dp], c_int),
            "cfp_group_apply": ([vp, P(vp), P(vp)], c_int),
            "cfp_group_set_schedule": ([vp, c_int], c_int),
            "cfp_dist_plan_set_schedule": ([vp, c_int], c_int),
            "cfp_slab_steps_count": ([i64, i64, i64, c_int, c_int, c_int, c_int, c_int, P(c_int)], c_int),
            "cfp_slab_steps_get": ([i64, i64, i64, c_int, c_int, c_int, c_int, c_int, c_int, P(i64), P(d)], c_int),
            "cfp_dist_plan_create_with_comm": ([P(vp), i64, i64, i64, c_int, c_int, vp, c_int], c_int),
            "cfp_dist_plan_set_exchange": ([vp, vp, vp], c_int),
            "cfp_dist_plan_set_work_buffers": ([vp, dp, dp], c_int),
            "cfp_dist_plan_num_steps": ([vp, P(c_int)], c_int),
            "cfp_dist_plan_step": ([vp, c_int, P(i64)], c_int),
            "cfp_dist_plan_run_step": ([vp, c_int, dp, dp, vp], c_int),
            "cfp_dist_plan_set_diag": ([vp, dp, vp], c_int),
            "cfp_dist_plan_clear_diag": ([vp], c_int),
            "cfp_dist_plan_forward": ([vp, dp, dp, vp], c_int),
            "cfp_dist_plan_backward": ([vp, dp, dp, vp], c_int),
            "cfp_dist_plan_set_pieces": ([vp, c_int], c_int),
            "cfp_dist_plan_pieces": ([vp, P(c_int)], c_int),
            "cfp_group_set_pieces": ([vp, c_int], c_int),
            "cfp_dist_plan_use_diag": ([vp, c_int], c_int),
            "cfp_dist_plan_set_symbol_advdiff": ([vp, dp, dp], c_int),
            "cfp_dist_plan_set_symbol_upwind": ([vp, dp, dp], c_int),
            "cfp_group_set_symbol_upwind": ([vp, dp, dp], c_int),
            "cfp_dist_plan_set_mid_kernel": ([vp, c_int], c_int),
            "cfp_dist_plan_mid_kernel": ([vp, P(c_int)], c_int),
            "cfp_group_set_symbol_advdiff": ([vp, dp, dp], c_int),
            "cfp_group_set_mid_kernel": ([vp, c_int], c_int),
            "cfp_group_mid_kernel": ([vp, P(c_int)], c_int),
            "cfp_slab_advdiff_z_table": ([c_int, c_int, dp, dp, dp], c_int),
        }),
        # the PETSc stand-in: communicators, Vec, Mat, PC, KSP
        ("petsc_mini.h", BOTH, {
            "MPI_Comm_size": ([c_int, P(c_int)], c_int),
            "MPI_Comm_rank": ([c_int, P(c_int)], c_int),
            "PetscMiniCommCreate": ([c_int, c_int, vp, P(c_int)], c_int),
            "PetscMiniCommCreateRCCL": ([c_int, c_int, cs, P(c_int)], c_int),
            "PetscMiniCommDestroy": ([P(c_int)], c_int),
            "PetscMiniSetCommWorld": ([c_int], c_int),
            "PetscMiniCommResolve": ([c_int, P(c_int)], c_int),
            "PetscMiniAllreduce": ([c_int, P(d), i64, c_int], c_int),
            "PetscMiniCommGetNCCL": ([c_int, P(vp)], c_int),
            "PetscMiniMatAIJGetFormat": ([vp, P(c_int)], c_int),
            "PetscMiniMatAIJDescribe": ([vp, P(AIJInfo)], c_int),
            "PetscErrorLastMessage": ([], cs),
            "PetscObjectStateGet": ([vp, P(i64)], c_int),
            "PetscObjectGetId": ([vp, P(i64)], c_int),
            "PetscMiniDeviceRead": ([vp, i64, P(d)], c_int),
            "VecMiniSetStream": ([vp], c_int),
            "VecCreateSeq": ([c_int, i64, P(vp)], c_int),
            "VecCreateSeqHIP": ([c_int, i64, P(vp)], c_int),
            "VecCreateSeqHIPWithArray": ([c_int, i64, i64, vp, P(vp)], c_int),
            "VecCreateMPI": ([c_int, i64, i64, P(vp)], c_int),
            "VecCreateMPIHIP": ([c_int, i64, i64, P(vp)], c_int),
            "VecCreateMPIHIPWithArray": ([c_int, i64, i64, i64, vp, P(vp)], c_int),
            "VecDuplicate": ([vp, P(vp)], c_int),
            "VecDestroy": ([P(vp)], c_int),
            "VecGetComm": ([vp, P(c_int)], c_int),
            "VecGetSize": ([vp, P(i64)], c_int),
            "VecGetLocalSize": ([vp, P(i64)], c_int),
            "VecGetOwnershipRange": ([vp, P(i64), P(i64)], c_int),
            "VecGetArray": ([vp, P(vp)], c_int),
            "VecRestoreArray": ([vp, P(vp)], c_int),
            "VecGetArrayRead": ([vp, P(vp)], c_int),
            "VecRestoreArrayRead": ([vp, P(vp)], c_int),
            "VecHIPGetArray": ([vp, P(vp)], c_int),
            "VecHIPRestoreArray": ([vp, P(vp)], c_int),
            "VecSet": ([vp, S], c_int),
            "VecSetValue": ([vp, i64, S, c_int], c_int),
            "VecAssemblyBegin": ([vp], c_int),
            "VecAssemblyEnd": ([vp], c_int),
            "VecCopy": ([vp, vp], c_int),
            "VecScale": ([vp, S], c_int),
            "VecShift": ([vp, S], c_int),
            "VecAXPY": ([vp, S, vp], c_int),
            "VecAYPX": ([vp, S, vp], c_int),
            "VecWAXPY": ([vp, S, vp, vp], c_int),
            "VecPointwiseDivide": ([vp, vp, vp], c_int),
            "VecPointwiseMult": ([vp, vp, vp], c_int),
            "VecDot": ([vp, vp, P(S)], c_int),
            "VecNorm": ([vp, c_int, P(d)], c_int),
            "VecMDot": ([vp, i64, P(vp), P(S)], c_int),
            "VecMAXPY": ([vp, i64, P(S), P(vp)], c_int),
            "VecMiniMAXPYNorm": ([vp, i64, P(S), P(vp), c_int, P(d)], c_int),
            "VecMiniMDotMAXPYNorm": ([vp, i64, P(d), P(vp), P(S), P(d)], c_int),
            "VecMiniMAXPYNormDeviceDots": ([vp, i64, P(d), P(vp), vp, P(S), P(d)], c_int),
            "MatCreateSeqAIJWithArrays": ([c_int, i64, i64, P(i64), P(i64), vp, P(vp)], c_int),
            "MatCreateFFT": ([c_int, i64, P(i64), cs, P(vp)], c_int),
            "MatCreateVecsFFTW": ([vp, P(vp), P(vp), P(vp)], c_int),
            "MatCreateAIJ": ([c_int, i64, i64, i64, i64, i64, vp, i64, vp, P(vp)], c_int),
            "MatSetValues": ([vp, i64, P(i64), i64, P(i64), vp, c_int], c_int),
            "MatAssemblyBegin": ([vp, c_int], c_int),
            "MatAssemblyEnd": ([vp, c_int], c_int),
            "MatGetComm": ([vp, P(c_int)], c_int),
            "MatGetSize": ([vp, P(i64), P(i64)], c_int),
            "MatGetLocalSize": ([vp, P(i64), P(i64)], c_int),
            "MatGetOwnershipRange": ([vp, P(i64), P(i64)], c_int),
            "PetscMiniMatMPIAIJGetHalo": ([vp, P(i64), P(i64)], c_int),
            "MatMult": ([vp, vp, vp], c_int),
            "MatMultTranspose": ([vp, vp, vp], c_int),
            "MatShift": ([vp, S], c_int),
            "MatDestroy": ([P(vp)], c_int),
            "PCCreate": ([c_int, P(vp)], c_int),
            "PCSetType": ([vp, cs], c_int),
            "PCSetOperators": ([vp, vp, vp], c_int),
            "PCShellSetContext": ([vp, vp], c_int),
            "PCShellGetContext": ([vp, P(vp)], c_int),
            "PCShellSetApply": ([vp, vp], c_int),
            "PCShellSetSetUp": ([vp, vp], c_int),
            "PCShellSetDestroy": ([vp, vp], c_int),
            "PCSetUp": ([vp], c_int),
            "PCApply": ([vp, vp, vp], c_int),
            "PCDestroy": ([P(vp)], c_int),
            "KSPCreate": ([c_int, P(vp)], c_int),
            "KSPSetType": ([vp, cs], c_int),
            "KSPSetTolerances": ([vp, d, d, d, i64], c_int),
            "KSPGMRESSetRestart": ([vp, i64], c_int),
            "KSPSetPCSide": ([vp, c_int], c_int),
            "KSPSetInitialGuessNonzero": ([vp, c_int], c_int),
            "KSPGetPC": ([vp, P(vp)], c_int),
            "KSPSetOperators": ([vp, vp, vp], c_int),
            "KSPSetUp": ([vp], c_int),
            "KSPSolve": ([vp, vp, vp], c_int),
            "KSPGetConvergedReason": ([vp, P(c_int)], c_int),
            "KSPGetIterationNumber": ([vp, P(i64)], c_int),
            "KSPGetResidualNorm": ([vp, P(d)], c_int),
            "KSPMiniGetPCApplyStats": ([vp, P(i64), P(d)], c_int),
            "KSPMiniSetUpWork": ([vp, vp], c_int),
            "KSPDestroy": ([P(vp)], c_int),
        }),
        # the reference-named boundary and the FFT matrix behind it
        ("pcshell_fft3d.h", BOTH, {
            "MatCreateFFTHIP": ([c_int, i64, P(i64), P(vp)], c_int),
            "MatFFTHIPGetPlan": ([vp, P(vp)], c_int),
            "MatFFTHIPGetDistPlan": ([vp, P(vp)], c_int),
            "MatFFTHIPGetSolveCounts": ([vp, P(i64), P(i64)], c_int),
            "MatFFTHIPGetFusedBACount": ([vp, P(i64)], c_int),
            "applyFFT3DPrecTransport": ([vp, vp, vp], c_int),
            "applyFFT3DPrecTransportBA": ([vp, c_int, vp, vp, vp], c_int),
            "setupFFTPrec3D": ([vp], c_int),
            "setupFFTPrec3DUpwind": ([vp], c_int),
            "destroyFFTPrec3D": ([vp], c_int),
            "getFFTPrec3DContext": ([i64, S, i64, S, S, S, S, S, S, S, S, S, P(C.FFTPrecTransportContext)], c_int),
            "FFTPrecTransportContextCreate": ([P(vp)], c_int),
            "FFTPrecTransportContextSetRemapBack": ([P(C.FFTPrecTransportContext), vp], c_int),
            "FFTPrecTransportContextGetRemapBack": ([P(C.FFTPrecTransportContext), P(vp)], c_int),
            "FFTPrecTransportContextDestroy": ([P(vp)], c_int),
            "solve_3D": ([vp, vp, vp, vp, vp, i64], c_int),
            "build_transport_col": ([vp, i64], c_int),
            "build_diag_mat_vec_3D": ([vp, vp, vp, vp, i64, i64, i64, S, S, S], c_int),
            "FftTransportSolver": ([i64, i64, i64, S, S, S, vp, vp, vp], c_int),
            "Fft3DTransportSolver": ([i64, i64, i64, S, S, S, S, S, S, S, vp, vp, vp], c_int),
            "Fft2DTransportSolver": ([i64, i64, S, S, S, S, S, vp, vp, vp], c_int),
            "Fft1DTransportSolver": ([i64, S, S, S, vp, vp, vp], c_int),
            "PetscFft3DTransportSolver": ([C.StructuredTransportContext, vp, vp], c_int),
        }),
        # the real-data plan behind a real-scalar FFT matrix (csrc/pcshell_fft3d_real.cpp; no header)
        ("pcshell_fft3d_real.cpp", REAL_BUILD, {
            "MatFFTHIPGetRealPlan": ([vp, P(vp)], c_int),
        }),
        # advection-diffusion: PCSHELL, direct solver, operator, time loops
        ("diffusion_equation.h", BOTH, {
            "getFFTPrec3DDiffusionContext": ([i64, S, i64, i64, i64, S, S, S, S, P(d), P(d),
                                              P(C.FFTPrecDiffusionContext)], c_int),
            "setupFFTPrec3DDiffusion": ([vp], c_int),
            "setupFFTPrec3DDiffusionUpwind": ([vp], c_int),
            "applyFFT3DPrecDiffusion": ([vp, vp, vp], c_int),
            "destroyFFTPrec3DDiffusion": ([vp], c_int),
            "PetscFft3DDiffusionSolver": ([C.StructuredDiffusionContext, vp, vp], c_int),
            "cfp_advdiff_csr": ([i64, i64, i64, P(d), d, P(d), d, c_int, d, P(i64), P(i64), P(d), P(i64)], c_int),
            "computeAdvectionDiffusionMatrixCartesianAIJ": ([c_int, i64, i64, i64, P(d), d, P(d), d, i64, P(vp)],
                                                            c_int),
            "cfp_advdiff_config_default": ([P(AdvDiffConfig), i64], None),
            "AdvectionDiffusionGMRES": ([P(AdvDiffConfig), P(AdvDiffResult), P(d)], c_int),
            "AdvectionDiffusionFFTDirect": ([P(AdvDiffConfig), P(AdvDiffResult), P(d)], c_int),
        }),
        # transport operator + GMRES time loop
        ("transport_equation.h", COMPLEX_BUILD, {
            "cfp_transport_csr": ([i64, i64, i64, P(d), d, P(d), c_int, d, P(i64), P(i64), P(d), P(i64)], c_int),
            "cfp_cartesian_min_ratio_vol_surf": ([c_int, P(d)], d),
            "computeDivergenceMatrixCartesian": ([i64, i64, i64, P(d), d, P(d), i64, P(vp)], c_int),
            "initial_conditions_shock_cartesian": ([i64, i64, i64, P(d), P(d), vp], c_int),
            "cfp_transport_config_default": ([P(TransportConfig), i64], None),
            "TransportEquationGMRES": ([P(TransportConfig), P(TransportResult), P(d)], c_int),
            "TransportEquationFFTDirect": ([P(TransportConfig), P(TransportResult), P(d)], c_int),
        }),
        # unstructured meshes, the PCSHELL remap and the mesh transport loop
        ("mesh_unstructured.h", COMPLEX_BUILD, {
            "cfp_mesh_read_gmsh": ([cs, P(vp)], c_int),
            "cfp_mesh_create": ([i64, P(d), i64, P(i64), P(i64), P(vp)], c_int),
            "cfp_mesh_destroy": ([vp], c_int),
            "cfp_mesh_info": ([vp, P(i64), P(i64), P(i64), P(d)], c_int),
            "cfp_mesh_cell_geometry": ([vp, P(d), P(d)], c_int),
            "cfp_mesh_min_ratio_vol_surf": ([vp, P(d)], c_int),
            "cfp_mesh_faces": ([vp, P(i64), P(i64), P(d), P(d)], c_int),
            "cfp_mesh_crude_matrix_cartesian": ([vp, i64, i64, i64, P(d), P(i64), P(i64), P(i64), P(d)], c_int),
            "cfp_mesh_transport_csr": ([vp, d, P(d), c_int, d, P(i64), P(i64), P(i64), P(d)], c_int),
            "MatCreateMeshCartesianRemap": ([vp, i64, i64, i64, P(d), P(vp), P(vp)], c_int),
            "getFFTPrec3DContextMesh": ([i64, S, S, S, S, vp, vp], c_int),
            "FFTPrec3DContextDestroyRemap": ([vp], c_int),
            "initial_conditions_shock_mesh": ([vp, vp], c_int),
            "TransportEquationGMRESMesh": ([vp, P(TransportConfig), P(TransportResult), P(d)], c_int),
        }),
        ("wave_system.h", COMPLEX_BUILD, {
            "cfp_wave_plan_create": ([P(vp), i64, i64, i64, c_int], c_int),
            "cfp_wave_plan_create_dim": ([P(vp), i64, i64, i64, c_int, c_int], c_int),
            "cfp_wave_plan_destroy": ([vp], c_int),
            "cfp_wave_plan_set_symbol": ([vp, P(d), d], c_int),
            "cfp_wave_plan_apply": ([vp, dp, dp, vp], c_int),
            "cfp_wave_plan_apply_dots": ([vp, dp, dp, vp, c_int, P(vp), dp, P(c_int)], c_int),
            "cfp_wave_plan_set_schedule": ([vp, c_int], c_int),
            "cfp_wave_plan_forward": ([vp, dp, dp, vp], c_int),
            "cfp_wave_plan_backward": ([vp, dp, dp, vp], c_int),
            "cfp_wave_plan_num_passes": ([vp, P(c_int)], c_int),
            "cfp_wave_plan_time_passes": ([vp, dp, dp, c_int, dp, vp], c_int),
            "cfp_wave_csr": ([i64, i64, i64, P(d), d, d, c_int, d, P(i64), P(i64), P(d), P(i64)], c_int),
            "cfp_wave_csr_dim": ([i64, i64, i64, c_int, P(d), d, d, c_int, d, P(i64), P(i64), P(d), P(i64)], c_int),
            "computeDivergenceMatrixWaveCartesian": ([i64, i64, i64, P(d), d, d, i64, P(vp)], c_int),
            "computeDivergenceMatrixWaveCartesianDim": ([i64, i64, i64, i64, P(d), d, d, i64, P(vp)], c_int),
            "initial_conditions_shock_wave": ([i64, i64, i64, P(d), P(d), vp], c_int),
            "applyFFT3DPrecWave": ([vp, vp, vp], c_int),
            "setupFFTPrec3DWave": ([vp], c_int),
            "destroyFFTPrec3DWave": ([vp], c_int),
            "cfp_wave_config_default": ([P(WaveConfig), i64], None),
            "cfp_wave_config_default_dim": ([P(WaveConfig), i64, c_int], None),
            "WaveSystemGMRES": ([P(WaveConfig), P(WaveResult), P(d)], c_int),
        }),
        # the real-data wave plan and its PCSHELL
        ("wave_system_real.h", BOTH, {
            "cfp_wave_rplan_supported": ([i64, i64, i64, c_int], c_int),
            "cfp_wave_rplan_create": ([P(vp), i64, i64, i64, c_int, c_int], c_int),
            "cfp_wave_rplan_destroy": ([vp], c_int),
            "cfp_wave_rplan_set_symbol": ([vp, P(d), d], c_int),
            "cfp_wave_rplan_apply": ([vp, dp, dp, vp], c_int),
            "cfp_wave_rplan_apply_strided": ([vp, dp, dp, c_int, vp], c_int),
            "cfp_wave_rplan_num_passes": ([vp, P(c_int)], c_int),
            "cfp_wave_rplan_time_passes": ([vp, dp, dp, c_int, c_int, P(d), vp], c_int),
            "setupFFTPrec3DWaveRealData": ([vp], c_int),
            "applyFFT3DPrecWaveRealData": ([vp, vp, vp], c_int),
            "destroyFFTPrec3DWaveRealData": ([vp], c_int),
        }),
    ]


def declare(L, S, build: str) -> None:
    """Give every function of the table that `build` (COMPLEX_BUILD or REAL_BUILD) holds its argtypes and
    restype on the loaded library L.  Strict: a missing name raises AttributeError."""
    for _group, where, sig in signatures(S):
        if where in (BOTH, build):
            for name, (args, res) in sig.items():
                fn = getattr(L, name)
                fn.argtypes, fn.restype = args, res
