"""ctypes binding of the gfx950 RNS backend (C ABI: include/ofhe_hip.h).

Host-side mirror of the reference's offload interface for the hot path:

* ``Context``   ~ ``PimManager::getPim`` (src/core/include/pim/PimManager.h:23-29):
  one per device, allocation and host<->device copies.
* ``NTTPlan``   ~ ``ChineseRemainderTransformFTT<NativeVector>`` with its
  ``PreCompute`` tables (transformnat-impl.h:575-763) plus the
  ``NativeVectorT`` element-wise ops (mubintvecnat.cpp:245-367) over
  [batch][tower][N] device buffers.
* ``BaseConverter`` ~ ``DCRTPolyImpl::ApproxSwitchCRTBasis`` (dcrtpoly-impl.h:1034-1063).
* ``approx_mod_up`` / ``approx_mod_down`` ~ ``DCRTPolyImpl::ApproxModUp`` /
  ``ApproxModDown`` (dcrtpoly-impl.h:1085-1175).
* ``KeySwitch`` ~ ``KeySwitchHYBRID`` (pke/lib/keyswitch/keyswitch-hybrid.cpp:325-482)
  with the tables of ``CryptoParametersRNS::PrecomputeCRTTables``; its
  ``fast_rotation`` / ``fast_rotation_ext`` ~ ``EvalFastRotation``
  (base-leveledshe.cpp:471-513) / ``EvalFastRotationExt``
  (ckksrns-leveledshe.cpp:402-457) for many keys over one digit set; its
  ``bsgs_transform`` (stages ``ext``, ``mult_ext_sum``, ``fast_rotation_ext_sum``) ~ one
  BSGS level of ``FHECKKSRNS::EvalLinearTransform`` (ckksrns-fhe.cpp:1484-1555).
* ``BaseConverter.switch_exact`` / ``expand_crt_basis`` / ``ScaleRound`` / ``BfvMult`` ~
  ``DCRTPolyImpl::SwitchCRTBasis`` / ``ExpandCRTBasis`` / ``ScaleAndRound``
  (dcrtpoly-impl.h:1178-1230, 1311-1358, 1876-1955) and ``LeveledSHEBFVRNS::EvalMult``
  for HPS / HPSPOVERQ (bfvrns-leveledshe.cpp:168-408); their tables come from
  ``bfv_tables.py``.
* ``BfvLevel`` ~ ``LeveledSHEBFVRNS::EvalMult`` / ``EvalSquare`` / ``RelinearizeCore`` for HPSPOVERQLEVELED
  with dropped levels (bfvrns-leveledshe.cpp:235-274, 367-382, 459-499, 845-899) and
  ``DCRTPolyImpl::ExpandCRTBasisQlHat`` (dcrtpoly-impl.h:1514-1534); its tables are a
  ``bfv_tables.LeveledTables``.
* ``Behz`` ~ ``DCRTPolyImpl::FastBaseConvqToBskMontgomery`` / ``FastRNSFloorq`` / ``FastBaseConvSK``
  (dcrtpoly-impl.h:2050-2208, 2212-2271, 2309-2411) and ``LeveledSHEBFVRNS::EvalMult`` for BEHZ
  (bfvrns-leveledshe.cpp:275-297, 383-403); its tables are a ``bfv_tables.BehzTables``.
* ``BfvDecrypt`` ~ ``PKEBFVRNS::Decrypt`` (bfvrns-pke.cpp:205-248): ``PKERNS::DecryptCore``
  (rns-pke.cpp:199-224), the two ``ScaleAndRound`` overloads to a ``NativePoly`` mod t
  (dcrtpoly-impl.h:1537-1814, 2005-2049), the one-tower ``MultiplyAndRound`` path, and
  ``DCRTPolyImpl::TimesQovert`` (dcrtpoly-impl.h:1015-1031); its tables are a ``bfv_tables.DecryptTables``.
* ``BgvDecrypt`` ~ ``PKEBGVRNS::Decrypt`` (bgvrns-pke.cpp:44-99): the ``DCRTPolyImpl::ModReduce`` chain
  Q_l -> q_0 (dcrtpoly-impl.h:792-812) in one kernel per 8 towers, ``NativeVectorT::Mod(t)``
  (mubintvecnat.cpp:139-166) and both of the reference's branches; its tables are built by the library from the
  moduli.  ``NTTPlan.decrypt_core`` ~ ``PKERNS::DecryptCore`` (rns-pke.cpp:199-224), which with ``coeff_out`` is
  ``PKECKKSRNS::Decrypt`` / ``PKERNS::Decrypt`` up to their last line; ``bgv_scaling_factor`` is the host
  arithmetic on ``scalingFactorInt`` (bgvrns-pke.cpp:62-69).
* ``KeySwitch.eval_mult`` / ``eval_square`` / ``relinearize`` / ``rescale`` ~ ``LeveledSHEBase::EvalMult`` /
  ``EvalSquare`` with an evaluation key and ``RelinearizeInPlace`` (base-leveledshe.cpp:199-372) and
  ``ModReduceInternalInPlace`` of CKKS and BGV (ckksrns-leveledshe.cpp:107-132, bgvrns-leveledshe.cpp:45-77).
* ``switch_modulus`` / ``NTTPlan.automorphism`` ~ ``NativeVectorT::SwitchModulus``
  (mubintvecnat.cpp:111-136) / ``PolyImpl::AutomorphismTransform`` (poly-impl.h:312-365).

Errors raise ``MathError`` (the analogue of ``lbcrypto::math_error`` thrown by
``OPENFHE_THROW``).  Pointers are plain integers (e.g. ``torch.Tensor.data_ptr()``)
and streams are ``hipStream_t`` values as integers (``torch.cuda.Stream.cuda_stream``).

There is no CPU fallback: if ``lib/libofhe_hip.so`` is missing this module
raises on first use.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libofhe_hip.so")

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p


# scheme of KeySwitch.eval_mult / rescale (OFHE_SHE_*)
SHE_CKKS, SHE_BGV = 0, 1


class MathError(RuntimeError):
    """Raised when a backend call returns a non-zero status (cf. lbcrypto::math_error)."""


_lib: Optional[ctypes.CDLL] = None

# name -> (restype, argtypes)
class Bsgs(ctypes.Structure):
    """ofhe_bsgs: one BSGS level of ofhe_hip_ks_bsgs_transform."""
    _fields_ = [("nbaby", ctypes.c_uint32), ("ngiant", ctypes.c_uint32),
                ("baby_index", ctypes.POINTER(ctypes.c_uint32)), ("giant_index", ctypes.POINTER(ctypes.c_uint32)),
                ("baby_key_b", ctypes.POINTER(ctypes.c_void_p)), ("baby_key_a", ctypes.POINTER(ctypes.c_void_p)),
                ("giant_key_b", ctypes.POINTER(ctypes.c_void_p)), ("giant_key_a", ctypes.POINTER(ctypes.c_void_p)),
                ("diag", ctypes.c_void_p), ("diag_stride", ctypes.c_uint64),
                ("present", ctypes.POINTER(ctypes.c_uint8))]


_SIGS = {
    "ofhe_hip_last_error": (ctypes.c_char_p, []),
    "ofhe_hip_version": (ctypes.c_char_p, []),
    "ofhe_hip_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "ofhe_hip_init": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "ofhe_hip_finalize": (ctypes.c_int, [_vp]),
    "ofhe_hip_alloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "ofhe_hip_free": (ctypes.c_int, [_vp, _vp]),
    "ofhe_hip_alloc_async": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), _vp]),
    "ofhe_hip_free_async": (ctypes.c_int, [_vp, _vp, _vp]),
    "ofhe_hip_host_alloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "ofhe_hip_host_free": (ctypes.c_int, [_vp, _vp]),
    "ofhe_hip_zero": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    "ofhe_hip_copy_to_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "ofhe_hip_copy_to_host": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "ofhe_hip_copy_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "ofhe_hip_sync": (ctypes.c_int, [_vp, _vp]),
    "ofhe_hip_event_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_event_record": (ctypes.c_int, [_vp, _vp]),
    "ofhe_hip_event_sync": (ctypes.c_int, [_vp]),
    "ofhe_hip_event_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_trim": (ctypes.c_int, [_vp, ctypes.c_size_t]),
    "ofhe_hip_plan_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, _u64p,
                                            ctypes.POINTER(_vp)]),
    "ofhe_hip_plan_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_plan_tune": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32]),
    "ofhe_hip_plan_create_ex": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, _u64p,
                                               _vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_plan_tables": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p]),
    "ofhe_hip_ntt_fwd": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ntt_inv": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modmul_vv": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modadd_vv": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modsub_vv": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modmul_scalar": (ctypes.c_int, [_vp, _vp, _u64p, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modadd_scalar": (ctypes.c_int, [_vp, _vp, _u64p, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modsub_scalar": (ctypes.c_int, [_vp, _vp, _u64p, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_modadd_scalar_at": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _u64p, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_fill_uniform": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, _vp]),
    "ofhe_hip_ntt_mul_intt": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ntt_mul_intt_stage": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bconv_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             _u64p, _u64p, _u64p, _u64p, ctypes.POINTER(_vp)]),
    "ofhe_hip_bconv_create_ex": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                _u64p, _u64p, _u64p, _u64p, _vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_bconv_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_approx_switch_crt_basis": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ntt_fwd_range": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "ofhe_hip_ntt_inv_range": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "ofhe_hip_approx_mod_up": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_approx_mod_down": (ctypes.c_int, [_vp, _vp, _vp, _u64p, ctypes.c_uint64, _vp, _vp,
                                                ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, _u64p, ctypes.c_uint32,
                                          _u64p, _u64p, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "ofhe_hip_ks_create_ex": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, _u64p,
                                             ctypes.c_uint32, _u64p, _u64p, ctypes.c_uint32, _vp,
                                             ctypes.POINTER(_vp)]),
    "ofhe_hip_ks_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_ks_digits": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32)]),
    "ofhe_hip_ks_precompute": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_fast_core_ext": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32,
                                                 _vp]),
    "ofhe_hip_ks_mod_down": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                            _vp]),
    "ofhe_hip_ks_core": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                        ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_fast_rotation_ext": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_vp),
                                                     ctypes.POINTER(_vp), _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_fast_rotation": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                 ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_vp),
                                                 ctypes.POINTER(_vp), _vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                                 _vp]),
    "ofhe_hip_ks_ext": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_mult_ext_sum": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                                _vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint8),
                                                ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_fast_rotation_ext_sum": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_vp),
                                                         ctypes.POINTER(_vp), _vp, ctypes.c_uint32, _vp, _vp,
                                                         ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_bsgs_transform": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.POINTER(Bsgs), _vp, _vp, _vp, _vp,
                                                  ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_rescale": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.c_uint32,
                                           _vp]),
    "ofhe_hip_ks_relinearize": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp),
                                               ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, ctypes.c_uint64,
                                               ctypes.c_uint32, _vp]),
    "ofhe_hip_ks_eval_mult": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                             ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_switch_modulus": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               _vp]),
    "ofhe_hip_automorphism": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_drop_last_and_scale": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                                    ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_mod_reduce": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                           ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_precompute": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_core": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                        ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_digit_count": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_precompute_digits": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                     _vp]),
    "ofhe_hip_bv_core_digits": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32,
                                               _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_key_switch": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32,
                                              _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]),
    "ofhe_hip_bv_tune": (ctypes.c_int, [ctypes.c_uint32]),
    "ofhe_hip_eval_mult_core": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_switch_crt_basis": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_expand_crt_basis": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_scale_round_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u64p,
                                                   _u64p, ctypes.c_int, _u64p, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(_vp)]),
    "ofhe_hip_scale_round_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_scale_and_round": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_mult_create": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                ctypes.POINTER(_vp)]),
    "ofhe_hip_bfv_mult_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_bfv_eval_mult": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_level_create": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                 _u64p, ctypes.POINTER(_vp)]),
    "ofhe_hip_bfv_level_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_expand_ql_hat": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_scale_round_expand_ql_hat": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_eval_mult_leveled": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32,
                                                      _vp]),
    "ofhe_hip_bfv_relinearize_leveled": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_int, _vp, _vp, _vp, _vp,
                                                        _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_behz_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, ctypes.c_uint32, _u64p,
                                            ctypes.c_uint64, _vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_behz_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_behz_q_to_bsk": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_behz_expand": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_behz_floor": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_behz_conv_sk": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_behz_floor_sk": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_eval_mult_behz": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_decrypt_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, ctypes.c_uint64,
                                                   ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_bfv_decrypt_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_bfv_decrypt_branch": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "ofhe_hip_bfv_decrypt_scale_round": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bfv_decrypt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_int, _vp, _vp, _vp, _vp, _vp,
                                            ctypes.c_uint32, _vp]),
    "ofhe_hip_times_q_over_t": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_bgv_decrypt_create": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p, ctypes.c_uint64,
                                                   ctypes.POINTER(_vp)]),
    "ofhe_hip_bgv_decrypt_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_bgv_mod_reduce_chain": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_int, _vp, _vp, ctypes.c_uint32,
                                                     _vp]),
    "ofhe_hip_bgv_decrypt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, _vp, _vp, _vp,
                                            _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_decrypt_core": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _vp,
                                             _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "ofhe_hip_comm_unique_id": (ctypes.c_int, [_vp]),
    "ofhe_hip_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "ofhe_hip_comm_destroy": (ctypes.c_int, [_vp]),
    "ofhe_hip_bcast_evalkey": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
}

COMM_ID_BYTES = 128  # OFHE_COMM_ID_BYTES
BEHZ_FUSED_MAX_B = 16  # OFHE_BEHZ_FUSED_MAX_B: most B towers of the fused floor -> SK launch
BGV_DECRYPT_MAX_TOWERS = 64  # OFHE_BGV_DECRYPT_MAX_TOWERS: most towers of a BgvDecrypt handle
BGV_CHAIN_K = 8  # towers one launch of the ModReduce chain retires (csrc/bgv_decrypt_kernels.hpp); more run in passes
KS_ROT_CAP = 16  # rotations per launch of the hoisted-rotation calls (csrc/ks_kernels.hpp); more run in chunks

EXPORTED_SYMBOLS = tuple(_SIGS)


def lib() -> ctypes.CDLL:
    """Load (once) and return the backend library; raise if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MathError(
                f"HIP backend not built: {LIB_PATH} is missing "
                "(run __graft_entry__.build() or make -C upmem--openfhe_amd/csrc)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = lib().ofhe_hip_last_error().decode(errors="replace")
        raise MathError(f"ofhe_hip error {rc}: {msg}")


def _arr(vals: Sequence[int]):
    return (ctypes.c_uint64 * len(vals))(*[int(v) for v in vals])


def _ptrs(v):
    """Host array of device pointers; None stays NULL, a 0 entry a NULL entry."""
    return None if v is None else (_vp * len(v))(*[int(p) or None for p in v])


def _c012(elements: Sequence[int]):
    """The C ABI's (c0, c1, c2) of a ciphertext of 2 or 3 device pointers: a missing c2 is NULL; the count is
    checked by the library."""
    c = [int(p) for p in elements] + [0] * (3 - len(elements))
    return [_vp(p or None) for p in c[:3]]


def version() -> str:
    return lib().ofhe_hip_version().decode()


def bv_digit_count(moduli: Sequence[int], digit_size: int) -> int:
    """CRTDecompose(digit_size)'s nWindows over `moduli` (dcrtpoly-impl.h:290-300), with no device: one digit
    per tower at 0, else ceil(bitlen(q_i) / digit_size) windows per tower."""
    r = int(digit_size)
    if not 0 <= r <= 30:
        raise MathError("digit_size must be at most 30 (the reference forms 1 << digitSize in an int)")
    return sum(-(-int(q).bit_length() // r) if r else 1 for q in moduli)


def bv_tune(key_stationary: int) -> None:
    """ofhe_hip_bv_tune: batch entries per thread of the BV inner product (0 auto, 1 plain, 2, 4)."""
    _check(lib().ofhe_hip_bv_tune(int(key_stationary)))


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(lib().ofhe_hip_device_count(ctypes.byref(n)))
    return n.value


# Kernel-choice options of include/ofhe_hip.h (ofhe_plan_options,
# ofhe_bconv_options, ofhe_ks_options).  Zero = the library's defaults; every
# setting gives the same results (tests reach every kernel through them).
SPLIT_AUTO, SPLIT_COLS, SPLIT_8_8, SPLIT_9_8, SPLIT_8_9 = range(5)
BCONV_KERNEL_AUTO, BCONV_KERNEL_LIMB, BCONV_KERNEL_WIDE = range(3)


class PlanOptions(ctypes.Structure):
    _fields_ = [("split", ctypes.c_uint32), ("generic_moduli", ctypes.c_uint32)]


class BconvOptions(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_uint32), ("separate_cols", ctypes.c_uint32)]


class KsOptions(ctypes.Structure):
    _fields_ = [("plan", PlanOptions), ("separate_cols", ctypes.c_uint32), ("separate_icol", ctypes.c_uint32),
                ("chunk", ctypes.c_uint32), ("single_stream", ctypes.c_uint32)]


def _opt_ptr(o):
    return None if o is None else ctypes.cast(ctypes.byref(o), _vp)


class _Handle:
    """Owner of the C-ABI handle in ``_h``: close() destroys it once, through the symbol the class names."""

    _destroy = ""
    _h = None

    def close(self) -> None:
        if self._h is not None:
            _check(getattr(lib(), self._destroy)(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """Per-device context (PimManager analogue)."""

    _destroy = "ofhe_hip_finalize"

    def __init__(self, device: int = 0):
        h = _vp()
        _check(lib().ofhe_hip_init(int(device), ctypes.byref(h)))
        self._h = h
        self.device = device

    @property
    def handle(self):
        if self._h is None:
            raise MathError("context finalized")
        return self._h

    def alloc(self, nbytes: int) -> int:
        p = _vp()
        _check(lib().ofhe_hip_alloc(self.handle, int(nbytes), ctypes.byref(p)))
        return p.value

    def free(self, ptr: int) -> None:
        _check(lib().ofhe_hip_free(self.handle, _vp(ptr)))

    def alloc_async(self, nbytes: int, stream: int = 0) -> int:
        p = _vp()
        _check(lib().ofhe_hip_alloc_async(self.handle, int(nbytes), ctypes.byref(p), _vp(stream or None)))
        return p.value

    def free_async(self, ptr: int, stream: int = 0) -> None:
        _check(lib().ofhe_hip_free_async(self.handle, _vp(ptr), _vp(stream or None)))

    def host_alloc(self, nbytes: int) -> int:
        """Pinned host memory (staging for host-buffer integrations)."""
        p = _vp()
        _check(lib().ofhe_hip_host_alloc(self.handle, int(nbytes), ctypes.byref(p)))
        return p.value

    def host_free(self, ptr: int) -> None:
        _check(lib().ofhe_hip_host_free(self.handle, _vp(ptr)))

    def zero(self, dst: int, nbytes: int, stream: int = 0) -> None:
        _check(lib().ofhe_hip_zero(self.handle, _vp(dst), int(nbytes), _vp(stream or None)))

    def copy_to_device(self, dst: int, src: int, nbytes: int, stream: int = 0) -> None:
        _check(lib().ofhe_hip_copy_to_device(self.handle, _vp(dst), _vp(src), int(nbytes), _vp(stream or None)))

    def copy_to_host(self, dst: int, src: int, nbytes: int, stream: int = 0) -> None:
        _check(lib().ofhe_hip_copy_to_host(self.handle, _vp(dst), _vp(src), int(nbytes), _vp(stream or None)))

    def copy_device(self, dst: int, src: int, nbytes: int, stream: int = 0) -> None:
        _check(lib().ofhe_hip_copy_device(self.handle, _vp(dst), _vp(src), int(nbytes), _vp(stream or None)))

    def sync(self, stream: int = 0) -> None:
        _check(lib().ofhe_hip_sync(self.handle, _vp(stream or None)))

    def trim(self, keep_bytes: int = 0) -> None:
        """Give the context's cached stream-ordered memory back to the device."""
        _check(lib().ofhe_hip_trim(self.handle, keep_bytes))


class NTTPlan(_Handle):
    """Device-resident NTT tables for N = 2**log_n and one modulus per tower.

    Data buffers are [batch][towers][N] uint64 residues in device memory.
    """

    _destroy = "ofhe_hip_plan_destroy"

    def __init__(self, ctx: Context, log_n: int, moduli: Sequence[int], roots: Sequence[int],
                 split: int = SPLIT_AUTO, generic_moduli: bool = False):
        if len(moduli) != len(roots):
            raise MathError("moduli and roots differ in length")
        self.ctx = ctx
        self.log_n = int(log_n)
        self.n = 1 << self.log_n
        self.moduli = [int(q) for q in moduli]
        self.roots = [int(r) for r in roots]
        self.towers = len(self.moduli)
        h = _vp()
        o = PlanOptions(int(split), 1 if generic_moduli else 0)
        _check(lib().ofhe_hip_plan_create_ex(ctx.handle, self.log_n, self.towers, _arr(self.moduli),
                                             _arr(self.roots), _opt_ptr(o), ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        if self._h is None:
            raise MathError("plan destroyed")
        return self._h

    def tune(self, chunk_batch: int = 0, streams: int = 1) -> None:
        """Chunking / stream knob of ntt_mul_intt (speed only; results are identical)."""
        _check(lib().ofhe_hip_plan_tune(self.handle, int(chunk_batch), int(streams)))

    def tables(self):
        """Host copies of (Table, TableP, TableI, TableIP, ninv) as flat lists."""
        tn = self.towers * self.n
        a, b, c, d = (ctypes.c_uint64 * tn)(), (ctypes.c_uint64 * tn)(), (ctypes.c_uint64 * tn)(), (ctypes.c_uint64 * tn)()
        e = (ctypes.c_uint64 * self.towers)()
        _check(lib().ofhe_hip_plan_tables(self.handle, a, b, c, d, e))
        return list(a), list(b), list(c), list(d), list(e)

    # --- transforms (ChineseRemainderTransformFTT) ---
    def forward(self, data: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ntt_fwd(self.handle, _vp(data), int(batch), _vp(stream or None)))

    def inverse(self, data: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ntt_inv(self.handle, _vp(data), int(batch), _vp(stream or None)))

    # --- NativeVectorT element-wise (vector, vector) ---
    def mod_mul(self, a: int, b: int, c: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_modmul_vv(self.handle, _vp(a), _vp(b), _vp(c), int(batch), _vp(stream or None)))

    def mod_add(self, a: int, b: int, c: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_modadd_vv(self.handle, _vp(a), _vp(b), _vp(c), int(batch), _vp(stream or None)))

    def mod_sub(self, a: int, b: int, c: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_modsub_vv(self.handle, _vp(a), _vp(b), _vp(c), int(batch), _vp(stream or None)))

    def mod_mul_scalar(self, a: int, scalars: Sequence[int], c: int, batch: int = 1, stream: int = 0) -> None:
        if len(scalars) != self.towers:
            raise MathError("one scalar per tower required")
        _check(lib().ofhe_hip_modmul_scalar(self.handle, _vp(a), _arr(scalars), _vp(c), int(batch),
                                            _vp(stream or None)))

    def mod_add_scalar(self, a: int, scalars: Sequence[int], c: int, batch: int = 1, stream: int = 0) -> None:
        """NativeVectorT::ModAdd(const IntegerType&) per tower (mubintvecnat.cpp:198-219)."""
        if len(scalars) != self.towers:
            raise MathError("one scalar per tower required")
        _check(lib().ofhe_hip_modadd_scalar(self.handle, _vp(a), _arr(scalars), _vp(c), int(batch),
                                            _vp(stream or None)))

    def mod_sub_scalar(self, a: int, scalars: Sequence[int], c: int, batch: int = 1, stream: int = 0) -> None:
        """NativeVectorT::ModSub(const IntegerType&) per tower (mubintvecnat.cpp:267-288)."""
        if len(scalars) != self.towers:
            raise MathError("one scalar per tower required")
        _check(lib().ofhe_hip_modsub_scalar(self.handle, _vp(a), _arr(scalars), _vp(c), int(batch),
                                            _vp(stream or None)))

    def mod_add_scalar_at(self, a: int, index: int, scalars: Sequence[int], c: int, batch: int = 1,
                          stream: int = 0) -> None:
        """NativeVectorT::ModAddAtIndex(index, s_t) per tower (mubintvecnat.cpp:221-231); only word
        `index` of each (batch, tower) of c is written."""
        if len(scalars) != self.towers:
            raise MathError("one scalar per tower required")
        _check(lib().ofhe_hip_modadd_scalar_at(self.handle, _vp(a), int(index), _arr(scalars), _vp(c), int(batch),
                                               _vp(stream or None)))

    def fill_uniform(self, dst: int, batch: int, seed: int, batch_offset: int = 0, stream: int = 0) -> None:
        """Synthetic residues: splitmix64 streams seeded 0x5EED ^ (b<<20) ^ (t<<8) ^ seed, mod q_t."""
        _check(lib().ofhe_hip_fill_uniform(self.handle, _vp(dst), int(batch), int(batch_offset), int(seed),
                                           _vp(stream or None)))

    # --- tower-range transforms on strided data ---
    def forward_range(self, t0: int, count: int, src: int, dst: int, src_stride: int, dst_stride: int,
                      batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ntt_fwd_range(self.handle, int(t0), int(count), _vp(src), _vp(dst), int(src_stride),
                                            int(dst_stride), int(batch), _vp(stream or None)))

    def inverse_range(self, t0: int, count: int, src: int, dst: int, src_stride: int, dst_stride: int,
                      batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ntt_inv_range(self.handle, int(t0), int(count), _vp(src), _vp(dst), int(src_stride),
                                            int(dst_stride), int(batch), _vp(stream or None)))

    def automorphism(self, k: int, eval_form: bool, src: int, dst: int, batch: int = 1, stream: int = 0) -> None:
        """PolyImpl::AutomorphismTransform(k) on every (batch, tower); dst must not alias src."""
        _check(lib().ofhe_hip_automorphism(self.handle, int(k), 1 if eval_form else 0, _vp(src), _vp(dst),
                                           int(batch), _vp(stream or None)))

    # --- rescaling (DCRTPolyImpl::DropLastElementAndScale / ModReduce) ---
    def drop_last_and_scale(self, towers: int, x: int, x_stride: int, out: int, out_stride: int, eval_form: bool,
                            ql_ql_inv_modql_divql_modq, ql_inv_modq, batch: int = 1, stream: int = 0) -> None:
        """dcrtpoly-impl.h:746-768 on [batch][towers] -> [batch][towers - 1] (out may be x with equal strides; other overlap is rejected)."""
        c, a = list(ql_ql_inv_modql_divql_modq), list(ql_inv_modq)
        if len(c) < towers - 1 or len(a) < towers - 1:
            raise MathError("need towers - 1 constants")
        _check(lib().ofhe_hip_drop_last_and_scale(self.handle, int(towers), _vp(x), int(x_stride), _vp(out),
                                                  int(out_stride), 1 if eval_form else 0, _arr(c), _arr(a), int(batch),
                                                  _vp(stream or None)))

    def mod_reduce(self, towers: int, x: int, x_stride: int, out: int, out_stride: int, eval_form: bool, t: int,
                   neg_t_inv_modq: int, ql_inv_modq, batch: int = 1, stream: int = 0) -> None:
        """dcrtpoly-impl.h:792-812 on [batch][towers] -> [batch][towers - 1] (out may be x with equal strides; other overlap is rejected)."""
        a = list(ql_inv_modq)
        if len(a) < towers - 1:
            raise MathError("need towers - 1 constants")
        _check(lib().ofhe_hip_mod_reduce(self.handle, int(towers), _vp(x), int(x_stride), _vp(out), int(out_stride),
                                         1 if eval_form else 0, int(t), int(neg_t_inv_modq), _arr(a), int(batch),
                                         _vp(stream or None)))

    # --- BV key switching, digitSize = 0 (keyswitch-bv.cpp:302-340) ---
    def bv_precompute(self, towers: int, c: int, digits: int, batch: int = 1, stream: int = 0) -> None:
        """CRTDecompose(0) of c [batch][towers][N] (evaluation form) -> digits [batch][towers][towers][N]."""
        _check(lib().ofhe_hip_bv_precompute(self.handle, int(towers), _vp(c), _vp(digits), int(batch),
                                            _vp(stream or None)))

    def bv_core(self, towers: int, digits: int, key_b: int, key_a: int, key_towers: int, out0: int, out1: int,
                batch: int = 1, stream: int = 0) -> None:
        """EvalFastKeySwitchCore: out0 = sum_i kb[i] d_i, out1 = sum_i ka[i] d_i."""
        _check(lib().ofhe_hip_bv_core(self.handle, int(towers), _vp(digits), _vp(key_b), _vp(key_a), int(key_towers),
                                      _vp(out0), _vp(out1), int(batch), _vp(stream or None)))

    # --- BV key switching with a digit size (CRTDecompose(r), dcrtpoly-impl.h:266-320); 0 = the calls above ---
    def bv_digit_count(self, towers: int, digit_size: int) -> int:
        """The reference's nWindows over the plan's first `towers` moduli."""
        n = ctypes.c_uint32(0)
        _check(lib().ofhe_hip_bv_digit_count(self.handle, int(towers), int(digit_size), ctypes.byref(n)))
        return n.value

    def bv_precompute_digits(self, towers: int, digit_size: int, c: int, digits: int, batch: int = 1,
                             stream: int = 0) -> None:
        """CRTDecompose(digit_size) of c [batch][towers][N] (evaluation form) -> digits [batch][n_digits][towers][N]."""
        _check(lib().ofhe_hip_bv_precompute_digits(self.handle, int(towers), int(digit_size), _vp(c), _vp(digits),
                                                   int(batch), _vp(stream or None)))

    def bv_core_digits(self, towers: int, n_digits: int, digits: int, key_b: int, key_a: int, key_towers: int,
                       out0: int, out1: int, batch: int = 1, stream: int = 0) -> None:
        """EvalFastKeySwitchCore over n_digits digits and the first n_digits polynomials of the keys."""
        _check(lib().ofhe_hip_bv_core_digits(self.handle, int(towers), int(n_digits), _vp(digits), _vp(key_b),
                                             _vp(key_a), int(key_towers), _vp(out0), _vp(out1), int(batch),
                                             _vp(stream or None)))

    def bv_key_switch(self, towers: int, digit_size: int, c: int, key_b: int, key_a: int, key_towers: int, add0: int,
                      add1: int, out0: int, out1: int, chunk_digits: int = 0, batch: int = 1, stream: int = 0) -> None:
        """KeySwitchInPlace: out0 = add0 + ct0, out1 = add1 + ct1 (an addend of 0 / None is zero), the digits
        produced and consumed chunk_digits at a time (0: the library's scratch bound)."""
        _check(lib().ofhe_hip_bv_key_switch(self.handle, int(towers), int(digit_size), _vp(c), _vp(key_b), _vp(key_a),
                                            int(key_towers), _vp(add0 or None), _vp(add1 or None), _vp(out0),
                                            _vp(out1), int(chunk_digits), int(batch), _vp(stream or None)))

    # --- PKERNS::DecryptCore (rns-pke.cpp:199-224) ---
    def decrypt_core(self, size_ql: int, elements: Sequence[int], s: int, out: int, eval_form: bool = True,
                     coeff_out: bool = False, batch: int = 1, stream: int = 0) -> None:
        """out = c0 + c1 s (+ c2 s^2) over the first size_ql towers; elements: the 2 or 3 device pointers, each
        [batch][size_ql][N]; coeff_out adds the INTT (PKECKKSRNS::Decrypt / PKERNS::Decrypt up to their last
        line).  out may be elements[0]."""
        _check(lib().ofhe_hip_decrypt_core(self.handle, int(size_ql), len(elements), 1 if eval_form else 0,
                                           1 if coeff_out else 0, *_c012(elements), _vp(s), _vp(out), int(batch),
                                           _vp(stream or None)))

    # --- LeveledSHEBase::EvalMultCore, 2 x 2 elements (base-leveledshe.cpp:667-672) ---
    def eval_mult_core(self, c0: int, c1: int, d0: int, d1: int, out0: int, out1: int, out2: int, batch: int = 1,
                       stream: int = 0) -> None:
        _check(lib().ofhe_hip_eval_mult_core(self.handle, _vp(c0), _vp(c1), _vp(d0), _vp(d1), _vp(out0), _vp(out1),
                                             _vp(out2), int(batch), _vp(stream or None)))

    # --- the metric pipeline ---
    def ntt_mul_intt(self, a: int, b: int, c: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ntt_mul_intt(self.handle, _vp(a), _vp(b), _vp(c), int(batch), _vp(stream or None)))


    def ntt_mul_intt_stage(self, stage: int, a: int, b: int, c: int, batch: int = 1, stream: int = 0) -> None:
        """One kernel of ntt_mul_intt (0: forward columns, 1: fused block pass, 2: inverse columns)."""
        _check(lib().ofhe_hip_ntt_mul_intt_stage(self.handle, int(stage), _vp(a), _vp(b), _vp(c), int(batch),
                                                 _vp(stream or None)))


class BaseConverter(_Handle):
    """ApproxSwitchCRTBasis from basis Q (size_q towers) to basis P (size_p towers)."""

    _destroy = "ofhe_hip_bconv_destroy"

    def __init__(self, ctx: Context, log_n: int, q: Sequence[int], p: Sequence[int],
                 qhat_inv_modq: Sequence[int], qhat_modp: Sequence[int], kernel: int = BCONV_KERNEL_AUTO,
                 separate_cols: bool = False):
        self.ctx = ctx
        self.log_n = int(log_n)
        self.size_q, self.size_p = len(q), len(p)
        if len(qhat_inv_modq) != self.size_q or len(qhat_modp) != self.size_q * self.size_p:
            raise MathError("precomputation sizes do not match the bases")
        h = _vp()
        o = BconvOptions(int(kernel), 1 if separate_cols else 0)
        _check(lib().ofhe_hip_bconv_create_ex(ctx.handle, self.log_n, self.size_q, self.size_p, _arr(q), _arr(p),
                                              _arr(qhat_inv_modq), _arr(qhat_modp), _opt_ptr(o), ctypes.byref(h)))
        self._h = h

    def switch(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_approx_switch_crt_basis(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def switch_exact(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        """DCRTPolyImpl::SwitchCRTBasis (dcrtpoly-impl.h:1178-1230): the exact switch with the
        floating-point overflow count; the converter must hold the true CRT tables."""
        _check(lib().ofhe_hip_switch_crt_basis(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))


def switch_modulus(ctx: Context, src: int, dst: int, n: int, old_q: int, new_q: int, stream: int = 0) -> None:
    """NativeVectorT::SwitchModulus on n words of device memory."""
    _check(lib().ofhe_hip_switch_modulus(ctx.handle, _vp(src), _vp(dst), int(n), int(old_q), int(new_q),
                                         _vp(stream or None)))


def approx_mod_up(plan_q: NTTPlan, plan_p: NTTPlan, q_to_p: BaseConverter, eval_form: bool, x: int, out: int,
                  batch: int = 1, stream: int = 0) -> None:
    """ApproxModUp: x [batch][Q][N] -> out [batch][Q+P][N] (evaluation form)."""
    _check(lib().ofhe_hip_approx_mod_up(plan_q.handle, plan_p.handle, q_to_p._h, 1 if eval_form else 0, _vp(x),
                                        _vp(out), int(batch), _vp(stream or None)))


def expand_crt_basis(plan_q: NTTPlan, plan_p: NTTPlan, q_to_p: BaseConverter, eval_form: bool, x: int, out: int,
                     batch: int = 1, stream: int = 0) -> None:
    """ExpandCRTBasis (dcrtpoly-impl.h:1311-1358, resultFormat = EVALUATION): x [batch][Q][N] -> out
    [batch][Q+P][N] (evaluation form) through the exact switch."""
    _check(lib().ofhe_hip_expand_crt_basis(plan_q.handle, plan_p.handle, q_to_p._h, 1 if eval_form else 0, _vp(x),
                                           _vp(out), int(batch), _vp(stream or None)))


class ScaleRound(_Handle):
    """DCRTPolyImpl::ScaleAndRound, DCRTPoly -> DCRTPoly (dcrtpoly-impl.h:1876-1955).  x is
    [batch][len(q) + len(p)][N], Q towers first, coefficient form; out_is_q = False (HPS) sums the Q
    towers into the P basis, True (HPSPOVERQ) the P towers into the Q basis.  int_table: size_o rows of
    size_i + 1 words (tOSHatInvModsDivsModo), frac: size_i doubles (tOSHatInvModsDivsFrac)."""

    _destroy = "ofhe_hip_scale_round_destroy"

    def __init__(self, ctx: Context, log_n: int, q: Sequence[int], p: Sequence[int], out_is_q: bool,
                 int_table: Sequence[Sequence[int]], frac: Sequence[float]):
        self.ctx, self.log_n = ctx, int(log_n)
        self.size_q, self.size_p, self.out_is_q = len(q), len(p), bool(out_is_q)
        si, so = (self.size_p, self.size_q) if out_is_q else (self.size_q, self.size_p)
        if len(int_table) != so or any(len(r) != si + 1 for r in int_table) or len(frac) != si:
            raise MathError("table sizes do not match the bases")
        self.size_i, self.size_o = si, so
        h = _vp()
        fr = (ctypes.c_double * si)(*[float(v) for v in frac])
        _check(lib().ofhe_hip_scale_round_create(ctx.handle, self.log_n, self.size_q, self.size_p, _arr(q), _arr(p),
                                                 1 if out_is_q else 0, _arr([v for r in int_table for v in r]), fr,
                                                 ctypes.byref(h)))
        self._h = h

    def run(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_scale_and_round(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))


BFV_HPS, BFV_HPSPOVERQ = range(2)


class BfvMult(_Handle):
    """LeveledSHEBFVRNS::EvalMult (bfvrns-leveledshe.cpp:168-408) for two 2-element ciphertexts, technique
    HPS or HPSPOVERQ, composed from the caller's handles (kept alive by this object).  q_to_r_neg (the
    mNegRlQHatInvModq / qInvModr converter) is None for HPS."""

    _destroy = "ofhe_hip_bfv_mult_destroy"

    def __init__(self, ctx: Context, technique: int, plan_q: NTTPlan, plan_r: NTTPlan, plan_qr: NTTPlan,
                 q_to_r: BaseConverter, r_to_q: BaseConverter, q_to_r_neg: Optional[BaseConverter],
                 scale_round: ScaleRound):
        self._parts = (ctx, plan_q, plan_r, plan_qr, q_to_r, r_to_q, q_to_r_neg, scale_round)
        h = _vp()
        _check(lib().ofhe_hip_bfv_mult_create(ctx.handle, int(technique), plan_q.handle, plan_r.handle,
                                              plan_qr.handle, q_to_r._h, r_to_q._h,
                                              None if q_to_r_neg is None else q_to_r_neg._h, scale_round._h,
                                              ctypes.byref(h)))
        self._h = h

    def eval_mult(self, c0: int, c1: int, d0: int, d1: int, out0: int, out1: int, out2: int, batch: int = 1,
                  stream: int = 0) -> None:
        """Inputs [batch][Q][N] evaluation form; outputs [batch][Q][N] coefficient form."""
        _check(lib().ofhe_hip_bfv_eval_mult(self._h, _vp(c0), _vp(c1), _vp(d0), _vp(d1), _vp(out0), _vp(out1),
                                            _vp(out2), int(batch), _vp(stream or None)))


class BfvLevel(_Handle):
    """One level l of HPSPOVERQLEVELED (l = the index of the last kept tower), composed from the
    caller's handles (kept alive by this object): plan_q over the full chain, plan_ql / plan_rl /
    plan_qlrl over Q_l, R_l and both, ql_to_rl / rl_to_ql with the true CRT tables, q_to_rl_neg (all
    size_q towers -> R_l with mNegRlQHatInvModq(l) / qInvModr), drop (ScaleRound Q -> Q_l, None at
    l = size_q - 1), scale_round (Q_l R_l -> Q_l) and ql_hat_modq ((Q / Q_l) mod q_i, i <= l).
    bfv_tables.LeveledTables holds every table."""

    _destroy = "ofhe_hip_bfv_level_destroy"

    def __init__(self, ctx: Context, l: int, plan_q: NTTPlan, plan_ql: NTTPlan, plan_rl: NTTPlan, plan_qlrl: NTTPlan,
                 ql_to_rl: BaseConverter, rl_to_ql: BaseConverter, q_to_rl_neg: BaseConverter,
                 drop: Optional[ScaleRound], scale_round: ScaleRound, ql_hat_modq: Sequence[int]):
        self._parts = (ctx, plan_q, plan_ql, plan_rl, plan_qlrl, ql_to_rl, rl_to_ql, q_to_rl_neg, drop, scale_round)
        self.l = int(l)
        if len(ql_hat_modq) != self.l + 1:
            raise MathError("ql_hat_modq must have l + 1 entries")
        h = _vp()
        _check(lib().ofhe_hip_bfv_level_create(ctx.handle, self.l, plan_q.handle, plan_ql.handle, plan_rl.handle,
                                               plan_qlrl.handle, ql_to_rl._h, rl_to_ql._h, q_to_rl_neg._h,
                                               None if drop is None else drop._h, scale_round._h,
                                               _arr(ql_hat_modq), ctypes.byref(h)))
        self._h = h

    def expand_ql_hat(self, x: int, out: int, addend: int = 0, batch: int = 1, stream: int = 0) -> None:
        """ExpandCRTBasisQlHat: x [batch][l + 1][N] -> out [batch][size_q][N], plus addend
        [batch][size_q][N] when given (out may be the addend's buffer)."""
        _check(lib().ofhe_hip_expand_ql_hat(self._h, _vp(x), _vp(addend or None), _vp(out), int(batch),
                                            _vp(stream or None)))

    def scale_round_expand(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        """ScaleAndRound Q_l R_l -> Q_l and ExpandCRTBasisQlHat in one launch: x [batch][2 (l + 1)][N]
        coefficient form -> out [batch][size_q][N]."""
        _check(lib().ofhe_hip_scale_round_expand_ql_hat(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def eval_mult(self, c0: int, c1: int, d0: int, d1: int, out0: int, out1: int, out2: int, batch: int = 1,
                  stream: int = 0) -> None:
        """Inputs [batch][size_q][N] evaluation form; outputs [batch][size_q][N] coefficient form."""
        _check(lib().ofhe_hip_bfv_eval_mult_leveled(self._h, _vp(c0), _vp(c1), _vp(d0), _vp(d1), _vp(out0),
                                                    _vp(out1), _vp(out2), int(batch), _vp(stream or None)))

    def eval_square(self, c0: int, c1: int, out0: int, out1: int, out2: int, batch: int = 1, stream: int = 0) -> None:
        """EvalSquare (bfvrns-leveledshe.cpp:459-499): the values of eval_mult(c, c)."""
        self.eval_mult(c0, c1, c0, c1, out0, out1, out2, batch, stream)

    def relinearize(self, ks: "KeySwitch", elements: Sequence[int], eval_form: bool, key_b: int, key_a: int,
                    out0: int, out1: int, batch: int = 1, stream: int = 0) -> None:
        """RelinearizeCore (bfvrns-leveledshe.cpp:845-899) of a 3- or 2-element ciphertext (device
        pointers in `elements`, [batch][size_q][N], all in one form); outputs in evaluation form."""
        if len(elements) not in (2, 3):
            raise MathError("a ciphertext of 2 or 3 elements is needed")
        c = [int(e) for e in elements] + [0]
        _check(lib().ofhe_hip_bfv_relinearize_leveled(self._h, ks._h, len(elements), 1 if eval_form else 0, _vp(c[0]),
                                                      _vp(c[1]), _vp(c[2] or None), _vp(key_b), _vp(key_a),
                                                      _vp(out0), _vp(out1), int(batch), _vp(stream or None)))


BEHZ_TWO_LAUNCHES, BEHZ_FUSED, BEHZ_AUTO = range(3)  # ofhe_hip_behz_floor_sk's `fused`


class BehzTablesStruct(ctypes.Structure):
    """ofhe_behz_tables: one host pointer per table, in the header's order"""
    _fields_ = [(name, _u64p) for name in (
        "tQHatInvModq", "QHatModbsk", "QHatModmtilde", "qInvModbsk", "mtildeQHatInvModq", "negQInvModmtilde",
        "QModbsk", "mtildeInvModbsk", "tQInvModbsk", "BHatInvModb", "BHatModq", "BHatModmsk", "BInvModmsk",
        "BModq")]


class Behz(_Handle):
    """The BEHZ variant of the BFV multiplication for ciphertext towers T.q, auxiliary towers T.b and
    T.msk (T: a ``bfv_tables.BehzTables``).  "Bsk" is the len(T.b) + 1 towers T.b + [T.msk].  Every
    array is [batch][towers][N] words of device memory.

    * ``q_to_bsk``   FastBaseConvqToBskMontgomery's conversion alone (dcrtpoly-impl.h:2098-2187):
      [Q] -> [Bsk], coefficient form.
    * ``expand``     the whole FastBaseConvqToBskMontgomery (2050-2208): [Q] -> [Q + Bsk], evaluation form.
    * ``floor``      FastRNSFloorq (2212-2271): [Q + Bsk] -> [Bsk], coefficient form.
    * ``conv_sk``    FastBaseConvSK (2309-2411) with the centred correction: [Bsk] -> [Q].
    * ``floor_sk``   the two in one launch (BEHZ_FUSED), in two (BEHZ_TWO_LAUNCHES) or as the
      multiplication chooses (BEHZ_AUTO): [Q + Bsk] -> [Q].
    * ``eval_mult``  LeveledSHEBFVRNS::EvalMult, BEHZ (bfvrns-leveledshe.cpp:275-297, 383-403)."""

    _destroy = "ofhe_hip_behz_destroy"

    def __init__(self, ctx: Context, log_n: int, T):
        self.ctx, self.log_n, self.tables = ctx, int(log_n), T
        self.size_q, self.size_b = len(T.q), len(T.b)
        self._keep = {name: _arr(T.flat(name)) for name in T.TABLES}
        ts = BehzTablesStruct(**{name: ctypes.cast(a, _u64p) for name, a in self._keep.items()})
        h = _vp()
        _check(lib().ofhe_hip_behz_create(ctx.handle, self.log_n, self.size_q, _arr(T.q), self.size_b, _arr(T.bsk),
                                          int(T.t), ctypes.cast(ctypes.byref(ts), _vp), ctypes.byref(h)))
        self._h = h

    def q_to_bsk(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_behz_q_to_bsk(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def expand(self, plan_q: NTTPlan, plan_bsk: NTTPlan, eval_form: bool, x: int, out: int, batch: int = 1,
               stream: int = 0) -> None:
        _check(lib().ofhe_hip_behz_expand(self._h, plan_q.handle, plan_bsk.handle, 1 if eval_form else 0, _vp(x),
                                          _vp(out), int(batch), _vp(stream or None)))

    def floor(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_behz_floor(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def conv_sk(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_behz_conv_sk(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def floor_sk(self, x: int, out: int, batch: int = 1, stream: int = 0, fused: int = BEHZ_AUTO) -> None:
        _check(lib().ofhe_hip_behz_floor_sk(self._h, int(fused), _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def eval_mult(self, plan_q: NTTPlan, plan_bsk: NTTPlan, plan_qbsk: NTTPlan, c0: int, c1: int, d0: int, d1: int,
                  out0: int, out1: int, out2: int, batch: int = 1, stream: int = 0) -> None:
        """Inputs [batch][Q][N] evaluation form; outputs [batch][Q][N] coefficient form."""
        _check(lib().ofhe_hip_bfv_eval_mult_behz(self._h, plan_q.handle, plan_bsk.handle, plan_qbsk.handle, _vp(c0),
                                                 _vp(c1), _vp(d0), _vp(d1), _vp(out0), _vp(out1), _vp(out2),
                                                 int(batch), _vp(stream or None)))


BFV_BEHZ = 2  # OFHE_BFV_BEHZ: BfvDecrypt's technique next to BFV_HPS / BFV_HPSPOVERQ
BFV_DECRYPT_BEHZ, BFV_DECRYPT_ONE_TOWER = 8, 9  # BfvDecrypt.branch after the loops A..H = 0..7


class BfvDecryptTablesStruct(ctypes.Structure):
    """ofhe_bfv_decrypt_tables: one host pointer per table, in the header's order"""
    _fields_ = [("tQHatInvModqDivqModt", _u64p), ("tQHatInvModqBDivqModt", _u64p),
                ("tQHatInvModqDivqFrac", ctypes.POINTER(ctypes.c_double)),
                ("tQHatInvModqBDivqFrac", ctypes.POINTER(ctypes.c_double)), ("tgammaQHatInvModq", _u64p),
                ("negInvqModtgamma", _u64p), ("tInvModq", _u64p), ("negQModt", _u64p)]


class BfvDecrypt(_Handle):
    """PKEBFVRNS::Decrypt (bfvrns-pke.cpp:205-248) and DCRTPolyImpl::TimesQovert for ciphertext towers T.q and
    plaintext modulus T.t (T: a ``bfv_tables.DecryptTables``), technique BFV_HPS / BFV_HPSPOVERQ or BFV_BEHZ.
    Tables the technique does not read, and members of T that are None, are not passed.

    * ``scale_round``      ScaleAndRound to t: x [batch][Q][N] coefficient form -> out [batch][N].
    * ``decrypt``          DecryptCore, INTT, ScaleAndRound: 2 or 3 elements [batch][Q][N] and the secret key
      [Q][N] (evaluation form) -> out [batch][N].
    * ``times_q_over_t``   TimesQovert over [batch][Q][N]; out may be x.
    * ``branch``           the loop that runs: 0..7 for A..H, BFV_DECRYPT_BEHZ, BFV_DECRYPT_ONE_TOWER."""

    _destroy = "ofhe_hip_bfv_decrypt_destroy"

    def __init__(self, ctx: Context, log_n: int, T, technique: int = BFV_HPS):
        self.ctx, self.log_n, self.tables, self.technique = ctx, int(log_n), T, int(technique)
        self.size_q = len(T.q)
        behz = self.technique == BFV_BEHZ
        names = ["tInvModq", "negQModt"]
        if self.size_q > 1:
            names += ["tgammaQHatInvModq", "negInvqModtgamma"] if behz else \
                ["tQHatInvModqDivqModt", "tQHatInvModqDivqFrac"] + \
                (["tQHatInvModqBDivqModt", "tQHatInvModqBDivqFrac"] if T.split else [])
        self._keep = {}
        for name in names:
            v = getattr(T, name)
            if v is None:
                continue
            if name.endswith("Frac"):
                self._keep[name] = (ctypes.c_double * len(v))(*[float(f) for f in v])
            else:
                self._keep[name] = _arr([v] if isinstance(v, int) else v)
        ts = BfvDecryptTablesStruct(**{n: ctypes.cast(a, dict(BfvDecryptTablesStruct._fields_)[n])
                                       for n, a in self._keep.items()})
        h = _vp()
        _check(lib().ofhe_hip_bfv_decrypt_create(ctx.handle if ctx is not None else None, self.log_n, self.size_q,
                                                 _arr(T.q), int(T.t), self.technique,
                                                 ctypes.cast(ctypes.byref(ts), _vp), ctypes.byref(h)))
        self._h = h

    @property
    def branch(self) -> int:
        b = ctypes.c_int(-1)
        _check(lib().ofhe_hip_bfv_decrypt_branch(self._h, ctypes.byref(b)))
        return b.value

    def scale_round(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_bfv_decrypt_scale_round(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))

    def decrypt(self, plan_q: NTTPlan, elements: Sequence[int], s: int, out: int, eval_form: bool, batch: int = 1,
                stream: int = 0) -> None:
        """elements: the 2 or 3 device pointers c0, c1 (, c2)."""
        _check(lib().ofhe_hip_bfv_decrypt(self._h, plan_q.handle, len(elements), 1 if eval_form else 0,
                                          *_c012(elements), _vp(s), _vp(out), int(batch), _vp(stream or None)))

    def times_q_over_t(self, x: int, out: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_times_q_over_t(self._h, _vp(x), _vp(out), int(batch), _vp(stream or None)))


class BgvDecrypt(_Handle):
    """PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) for ciphertext towers `moduli` and plaintext modulus t; the
    library builds negtInvModq and qlInvModq (bgvrns-cryptoparameters.cpp:91-107) from them.

    * ``mod_reduce_chain``  the ModReduce steps Q_l -> q_0 of a coefficient-form x [batch][size_ql][N] ->
      out [batch][N]: x_0 mod q_0, or with ``to_plaintext`` NativeVectorT::Mod(t) of it.
    * ``decrypt``           2 or 3 elements [batch][size_ql][N] and the secret key [size_q][N] (evaluation form)
      -> out [batch][N]; evaluation-form and coefficient-form elements take the reference's two branches."""

    _destroy = "ofhe_hip_bgv_decrypt_destroy"

    def __init__(self, ctx: Context, log_n: int, moduli: Sequence[int], t: int):
        self.ctx, self.log_n, self.t = ctx, int(log_n), int(t)
        self.moduli = [int(q) for q in moduli]
        self.size_q = len(self.moduli)
        h = _vp()
        _check(lib().ofhe_hip_bgv_decrypt_create(ctx.handle if ctx is not None else None, self.log_n, self.size_q,
                                                 _arr(self.moduli), self.t, ctypes.byref(h)))
        self._h = h

    def mod_reduce_chain(self, size_ql: int, x: int, out: int, to_plaintext: bool, batch: int = 1,
                         stream: int = 0) -> None:
        _check(lib().ofhe_hip_bgv_mod_reduce_chain(self._h, int(size_ql), 1 if to_plaintext else 0, _vp(x), _vp(out),
                                                   int(batch), _vp(stream or None)))

    def decrypt(self, plan_q: NTTPlan, size_ql: int, elements: Sequence[int], s: int, out: int, eval_form: bool,
                batch: int = 1, stream: int = 0) -> None:
        """elements: the 2 or 3 device pointers c0, c1 (, c2)."""
        _check(lib().ofhe_hip_bgv_decrypt(self._h, plan_q.handle, int(size_ql), len(elements), 1 if eval_form else 0,
                                          *_c012(elements), _vp(s), _vp(out), int(batch), _vp(stream or None)))


def bgv_scaling_factor(scaling_factor_int: int, mod_reduce_factors: Sequence[int], size_ql: int, t: int) -> int:
    """The scalingFactorInt PKEBGVRNS::Decrypt returns under FLEXIBLEAUTO / FLEXIBLEAUTOEXT (bgvrns-pke.cpp:62-69,
    82-89; the same in both branches), on the host: the ciphertext's factor times the inverse mod t of
    mod_reduce_factors[size_ql - 1 - i] for i < size_ql - 1, where mod_reduce_factors[l] is the caller's
    GetModReduceFactorInt(l).  Under the FIXED techniques the reference returns the factor unchanged."""
    t, sf, size_ql = int(t), int(scaling_factor_int), int(size_ql)
    if t < 2 or size_ql < 1 or (size_ql > 1 and len(mod_reduce_factors) < size_ql):
        raise MathError("bgv_scaling_factor: t >= 2 and one factor per level below size_ql expected")
    for i in range(size_ql - 1):
        f = int(mod_reduce_factors[size_ql - 1 - i]) % t
        try:
            inv = pow(f, -1, t)
        except ValueError:
            raise MathError(f"bgv_scaling_factor: factor {size_ql - 1 - i} is not invertible mod t") from None
        sf = sf % t * inv % t
    return sf


def approx_mod_down(plan_q: NTTPlan, plan_p: NTTPlan, p_to_q: BaseConverter, p_inv_modq: Sequence[int], t: int,
                    x: int, out: int, batch: int = 1, stream: int = 0) -> None:
    """ApproxModDown: x [batch][Q+P][N] -> out [batch][Q][N] (evaluation form)."""
    if len(p_inv_modq) != plan_q.towers:
        raise MathError("p_inv_modq needs one entry per Q tower")
    _check(lib().ofhe_hip_approx_mod_down(plan_q.handle, plan_p.handle, p_to_q._h, _arr(p_inv_modq), int(t),
                                          _vp(x), _vp(out), int(batch), _vp(stream or None)))


class KeySwitch(_Handle):
    """HYBRID key switching for ring 2**log_n, ciphertext moduli q (with roots
    rq), special moduli p (roots rp) and num_part_q digits."""

    _destroy = "ofhe_hip_ks_destroy"

    def __init__(self, ctx: Context, log_n: int, q: Sequence[int], rq: Sequence[int], p: Sequence[int],
                 rp: Sequence[int], num_part_q: int, options: "KsOptions" = None):
        self.ctx = ctx
        self.log_n, self.n = int(log_n), 1 << int(log_n)
        self.q, self.p = [int(v) for v in q], [int(v) for v in p]
        self.size_q, self.size_p = len(self.q), len(self.p)
        self.num_part_q = int(num_part_q)
        h = _vp()
        self.options = options
        _check(lib().ofhe_hip_ks_create_ex(ctx.handle, self.log_n, self.size_q, _arr(q), _arr(rq), self.size_p,
                                           _arr(p), _arr(rp), self.num_part_q, _opt_ptr(options), ctypes.byref(h)))
        self._h = h

    def digits(self, size_ql: int):
        """(alpha, beta) at level size_ql."""
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().ofhe_hip_ks_digits(self._h, int(size_ql), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def precompute(self, size_ql: int, c: int, digits: int, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ks_precompute(self._h, int(size_ql), _vp(c), _vp(digits), int(batch),
                                            _vp(stream or None)))

    def fast_core_ext(self, size_ql: int, digits: int, key_b: int, key_a: int, ct0: int, ct1: int,
                      batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ks_fast_core_ext(self._h, int(size_ql), _vp(digits), _vp(key_b), _vp(key_a),
                                               _vp(ct0), _vp(ct1), int(batch), _vp(stream or None)))

    def mod_down(self, size_ql: int, x: int, out: int, t: int = 0, batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ks_mod_down(self._h, int(size_ql), _vp(x), _vp(out), int(t), int(batch),
                                          _vp(stream or None)))

    def core(self, size_ql: int, c: int, key_b: int, key_a: int, out0: int, out1: int, t: int = 0,
             batch: int = 1, stream: int = 0) -> None:
        _check(lib().ofhe_hip_ks_core(self._h, int(size_ql), _vp(c), _vp(key_b), _vp(key_a), _vp(out0),
                                      _vp(out1), int(t), int(batch), _vp(stream or None)))

    @staticmethod
    def _rot_args(auto_indices, key_b_ptrs, key_a_ptrs):
        """(nrot, index array, key pointer arrays) of the hoisted-rotation calls; None stays NULL."""
        for v in (key_b_ptrs, key_a_ptrs):
            if auto_indices is not None and v is not None and len(v) != len(auto_indices):
                raise MathError("one evaluation key per automorphism index required")
        if auto_indices is None:
            return 0, None, _ptrs(key_b_ptrs), _ptrs(key_a_ptrs)
        for k in auto_indices:
            if not 0 <= int(k) < 1 << 32:
                raise MathError("automorphism index must fit 32 bits")
        idx = (ctypes.c_uint32 * len(auto_indices))(*[int(k) for k in auto_indices])
        return len(auto_indices), idx, _ptrs(key_b_ptrs), _ptrs(key_a_ptrs)

    def fast_rotation_ext(self, size_ql: int, digits: int, c0: int, auto_indices: Sequence[int],
                          key_b_ptrs: Sequence[int], key_a_ptrs: Sequence[int], out0: int, out1: int,
                          batch: int = 1, stream: int = 0) -> None:
        """LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:402-457) for every index of
        auto_indices over one digit set (precompute's output); c0 = 0: addFirst = false.
        out0, out1: [nrot][batch][size_ql + size_p][N]."""
        n, idx, kb, ka = self._rot_args(auto_indices, key_b_ptrs, key_a_ptrs)
        _check(lib().ofhe_hip_ks_fast_rotation_ext(self._h, int(size_ql), _vp(digits), _vp(c0 or None), n, idx, kb,
                                                   ka, _vp(out0), _vp(out1), int(batch), _vp(stream or None)))

    def fast_rotation(self, size_ql: int, digits: int, c0: int, auto_indices: Sequence[int],
                      key_b_ptrs: Sequence[int], key_a_ptrs: Sequence[int], out0: int, out1: int, t: int = 0,
                      batch: int = 1, stream: int = 0) -> None:
        """LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:471-513) for every index of auto_indices
        over one digit set.  out0, out1: [nrot][batch][size_ql][N]."""
        n, idx, kb, ka = self._rot_args(auto_indices, key_b_ptrs, key_a_ptrs)
        _check(lib().ofhe_hip_ks_fast_rotation(self._h, int(size_ql), _vp(digits), _vp(c0 or None), n, idx, kb, ka,
                                               _vp(out0), _vp(out1), int(t), int(batch), _vp(stream or None)))

    @staticmethod
    def _present(present, count):
        """Host byte array of the diagonals that exist; None stays NULL (all present)."""
        if present is None:
            return None
        if len(present) != count:
            raise MathError("present needs one entry per diagonal")
        return (ctypes.c_uint8 * count)(*[1 if v else 0 for v in present])

    def ext(self, size_ql: int, c: int, out: int, batch: int = 1, stream: int = 0) -> None:
        """KeySwitchHYBRID::KeySwitchExt (keyswitch-hybrid.cpp:231-256) on one element:
        c [batch][size_ql][N] -> out [batch][size_ql + size_p][N]."""
        _check(lib().ofhe_hip_ks_ext(self._h, int(size_ql), _vp(c or None), _vp(out or None), int(batch),
                                     _vp(stream or None)))

    def mult_ext_sum(self, size_ql: int, nterm: int, x0: int, x1: int, x_stride: int, diag: int, diag_stride: int,
                     present, nsum: int, out0: int, out1: int, batch: int = 1, stream: int = 0) -> None:
        """out_e[j] = sum_i x_e[i] * diag[j * nterm + i] over Ql|P (EvalMultExt / EvalAddExtInPlace,
        ckksrns-fhe.cpp:1520-1526); present: nsum * nterm truth values or None."""
        _check(lib().ofhe_hip_ks_mult_ext_sum(self._h, int(size_ql), int(nterm), _vp(x0 or None), _vp(x1 or None),
                                              int(x_stride), _vp(diag or None), int(diag_stride),
                                              self._present(present, int(nsum) * int(nterm)), int(nsum),
                                              _vp(out0 or None), _vp(out1 or None), int(batch),
                                              _vp(stream or None)))

    def fast_rotation_ext_sum(self, size_ql: int, digits: int, auto_indices: Sequence[int],
                              key_b_ptrs: Sequence[int], key_a_ptrs: Sequence[int], addend1: int, nadd: int,
                              out0: int, out1: int, batch: int = 1, stream: int = 0) -> None:
        """Sum over the digit sets of EvalFastRotationExt(., k_j, digits_j, false) under key j
        (ckksrns-fhe.cpp:1544-1545), plus nadd addends on element 1.  digits:
        [nset][batch][beta][size_ql + size_p][N]; out0, out1: [batch][size_ql + size_p][N]."""
        n, idx, kb, ka = self._rot_args(auto_indices, key_b_ptrs, key_a_ptrs)
        _check(lib().ofhe_hip_ks_fast_rotation_ext_sum(self._h, int(size_ql), n, _vp(digits or None), idx, kb, ka,
                                                       _vp(addend1 or None), int(nadd), _vp(out0 or None),
                                                       _vp(out1 or None), int(batch), _vp(stream or None)))

    def bsgs_transform(self, size_ql: int, baby_indices: Sequence[int], giant_indices: Sequence[int],
                       baby_key_b: Sequence[int], baby_key_a: Sequence[int], giant_key_b: Sequence[int],
                       giant_key_a: Sequence[int], diag: int, diag_stride: int, present, c0: int, c1: int,
                       out0: int, out1: int, t: int = 0, batch: int = 1, stream: int = 0) -> None:
        """One BSGS level of FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1484-1555): see
        ofhe_hip_ks_bsgs_transform.  Key pointers of identity steps (index = 1 mod 2N) may be 0."""
        nb, bi, bkb, bka = self._rot_args(baby_indices, baby_key_b, baby_key_a)
        ng, gi, gkb, gka = self._rot_args(giant_indices, giant_key_b, giant_key_a)
        tr = Bsgs(nb, ng, bi, gi, bkb, bka, gkb, gka, _vp(diag or None), int(diag_stride),
                  self._present(present, nb * ng))
        _check(lib().ofhe_hip_ks_bsgs_transform(self._h, int(size_ql), ctypes.byref(tr), _vp(c0 or None),
                                                _vp(c1 or None), _vp(out0 or None), _vp(out1 or None), int(t),
                                                int(batch), _vp(stream or None)))

    def eval_mult(self, size_ql: int, c0: int, c1: int, d0: int, d1: int, key_b: int, key_a: int, out0: int,
                  out1: int, scheme: int = SHE_CKKS, t: int = 0, levels: int = 0, batch: int = 1,
                  stream: int = 0) -> None:
        """LeveledSHEBase::EvalMult(ct1, ct2, evalKey) (base-leveledshe.cpp:199-259) followed by ``levels``
        rescalings (ModReduceInternalInPlace of the scheme); d0 = d1 = 0: EvalSquare.  out0, out1:
        [batch][size_ql - levels][N]."""
        _check(lib().ofhe_hip_ks_eval_mult(self._h, int(size_ql), _vp(c0 or None), _vp(c1 or None), _vp(d0 or None),
                                           _vp(d1 or None), _vp(key_b or None), _vp(key_a or None), int(scheme),
                                           int(t), int(levels), _vp(out0 or None), _vp(out1 or None), int(batch),
                                           _vp(stream or None)))

    def eval_square(self, size_ql: int, c0: int, c1: int, key_b: int, key_a: int, out0: int, out1: int,
                    scheme: int = SHE_CKKS, t: int = 0, levels: int = 0, batch: int = 1, stream: int = 0) -> None:
        """LeveledSHEBase::EvalSquare(ct, evalKey) (base-leveledshe.cpp:262-319), then ``levels`` rescalings."""
        self.eval_mult(size_ql, c0, c1, 0, 0, key_b, key_a, out0, out1, scheme, t, levels, batch, stream)

    def relinearize(self, size_ql: int, elements: Sequence[int], key_b_ptrs: Sequence[int],
                    key_a_ptrs: Sequence[int], out0: int, out1: int, t: int = 0, batch: int = 1,
                    stream: int = 0) -> None:
        """LeveledSHEBase::RelinearizeInPlace (base-leveledshe.cpp:357-372) of len(elements) >= 3 elements
        under len(elements) - 2 keys; out0 may be elements[0], out1 elements[1]."""
        n = 0 if elements is None else len(elements)
        for v in (key_b_ptrs, key_a_ptrs):
            if v is not None and elements is not None and n >= 2 and len(v) != n - 2:
                raise MathError("one evaluation key per element past the second required")
        _check(lib().ofhe_hip_ks_relinearize(self._h, int(size_ql), n, _ptrs(elements), _ptrs(key_b_ptrs),
                                             _ptrs(key_a_ptrs), _vp(out0 or None), _vp(out1 or None), int(t),
                                             int(batch), _vp(stream or None)))

    def rescale(self, size_ql: int, x_ptrs: Sequence[int], out_ptrs: Sequence[int], scheme: int = SHE_CKKS,
                t: int = 0, levels: int = 1, batch: int = 1, stream: int = 0) -> None:
        """ModReduceInternalInPlace (ckksrns-leveledshe.cpp:107-132, bgvrns-leveledshe.cpp:45-77): ``levels``
        rescalings of every element; out_ptrs[k]: [batch][size_ql - levels][N]."""
        if x_ptrs is not None and out_ptrs is not None and len(x_ptrs) != len(out_ptrs):
            raise MathError("one output per element required")
        n = 0 if x_ptrs is None else len(x_ptrs)
        _check(lib().ofhe_hip_ks_rescale(self._h, int(size_ql), int(scheme), int(t), int(levels), n,
                                         _ptrs(x_ptrs), _ptrs(out_ptrs), int(batch), _vp(stream or None)))


def comm_unique_id() -> bytes:
    """Rank 0's RCCL unique id (OFHE_COMM_ID_BYTES), to be sent to the others."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib().ofhe_hip_comm_unique_id(buf))
    return buf.raw


class Comm(_Handle):
    """RCCL communicator of this process's device (ofhe_hip_comm_init).
    Collective: every rank constructs it with the same id."""

    _destroy = "ofhe_hip_comm_destroy"

    def __init__(self, ctx: Context, nranks: int, rank: int, uid: bytes):
        if len(uid) != COMM_ID_BYTES:
            raise MathError(f"unique id must be {COMM_ID_BYTES} bytes")
        h = _vp()
        buf = ctypes.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _check(lib().ofhe_hip_comm_init(ctx.handle, int(nranks), int(rank), buf, ctypes.byref(h)))
        self._h, self._ctx, self.nranks, self.rank = h, ctx, nranks, rank

    def bcast_evalkey(self, key_ptr: int, words: int, root: int = 0, stream: int = 0) -> None:
        """In-place broadcast of `words` u64 of device memory from `root`."""
        if self._h is None:
            raise MathError("communicator destroyed")
        _check(lib().ofhe_hip_bcast_evalkey(self._h, _vp(key_ptr or None), int(words), int(root),
                                            _vp(stream or None)))

