"""dpgo_amd -- MI355X-native DPGO hot path (ctypes binding of libdpgo_amd.so).

The host-side mirror of the reference's C++ interface for the per-node MM / AMM
inner step of ``dist_pgo``:

  reference (C++/DPGO/include/DPGO)              here
  ---------------------------------------------  --------------------------------
  DPGO::read_g2o            DPGO_utils.h:49-51    read_g2o(filename, num_nodes) -> Graph
  DPGO::Options             DPGO_types.h:78-201   Options (same field names/defaults)
  DPGOHash(node, meas, opt) DPGOHash.h:13-107     NodeGroup(graph, node_ids, opt)[k] -> DPGOHash view
    initialize/update/iterate/communicate           same names, return 0 / -1
    results()               DPGO_types.h:204-322  .results() (scalars), .Xk(), .Xak()
  dist_pgo driver loop      dist_pgo.cpp:446-531  DistPGO
  DPGO::PCM                 PCM.h:10-71           PCM(device).update(graph, alpha, beta, X) / solve_exact / ...;
                                                  pcm_inliers(graph, X) -> keep mask, Graph.filter_edges(keep)
  SESyncProblem::verify_solution                  NodeGroup.certify(X) -> (CertResult, x); cert_lambda, cert_apply
                            SESyncProblem.cpp:375-468, SESync_utils.cpp:721-830 (fast_verification STEP 2)
  fast_verification         SESync_utils.cpp:721-830  NodeGroup.verify(X) -> (CertResult, x, CertFactor); cert_factor (STEP 1
                                                  alone: the device Cholesky of S + eta I), cert_matrix
  DPGOProblem::evaluate_E   DPGOProblem.cpp:634-681  EdgeEval(graph).run(X, loss, loss_reg): s_rot, s_trans, rho, w of EVERY
                                                  edge at a global X; Graph.scale_edges(w); verify_reweighted(graph, X,
                                                  loss, loss_reg): the certificate of the problem re-weighted at X

All compute runs in hand-written HIP kernels behind the C ABI of
include/dpgo_amd.h.  There is NO CPU fallback: creating a NodeGroup without a
HIP device raises.  numpy is used only to hold host matrices.
"""
from __future__ import annotations

import ctypes as C
import os

import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (DPGO_AMD_LIB: A/B builds of the same library from tools/build_variant.sh; never a different implementation)
LIB_PATH = os.environ.get("DPGO_AMD_LIB") or os.path.join(_HERE, "libdpgo_amd.so")

LOSS_NONE, LOSS_HUBER, LOSS_GM, LOSS_WELSCH = 0, 1, 2, 3
LOSS_NAMES = {"trivial": 0, "none": 0, "huber": 1, "gm": 2, "welsch": 3}
SCHEME_MM, SCHEME_AMM = 0, 1
RESCALE_STATIC, RESCALE_DYNAMIC = 0, 1
PRECON_NONE, PRECON_JACOBI, PRECON_ICHOL, PRECON_REG_CHOLESKY = 0, 1, 2, 3


class Options(C.Structure):
    """DPGO::Options (C++/DPGO/include/DPGO/DPGO_types.h:78-201)."""
    _fields_ = [
        ("scheme", C.c_int), ("regularizer", C.c_double), ("accepted_delta", C.c_double),
        ("eta", C.c_double * 2), ("psi", C.c_double), ("phi", C.c_double),
        ("max_soft_restart_hits", C.c_int * 2), ("oscillation_cnt_period", C.c_int),
        ("max_oscillations", C.c_int), ("loss", C.c_int), ("loss_reg", C.c_double),
        ("rescale", C.c_int), ("max_rescale_count", C.c_int), ("grad_norm_tol", C.c_double), ("rel_func_decrease_tol", C.c_double), ("stepsize_tol", C.c_double),
        ("max_iterations", C.c_int), ("max_iterations_accepted", C.c_int),
        ("reg_Cholesky_precon_max_condition_number", C.c_double),
        ("preconditioned_grad_norm_tol", C.c_double), ("max_tCG_iterations", C.c_int),
        ("STPCG_kappa", C.c_double), ("STPCG_theta", C.c_double), ("preconditioner", C.c_int),
        ("verbose", C.c_int),
    ]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_options_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    @staticmethod
    def driver(loss=LOSS_NONE, accelerated=True, **kw):
        """The hard-coded options of C++/examples/dist_pgo.cpp:103-120."""
        o = Options()
        lib().dpgo_options_driver(C.byref(o), int(loss), int(bool(accelerated)))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def p2p_plan(rank, exported, needed):
    """The neighbour-to-neighbour exchange plan of `rank` (comm.cpp::p2p_plan through dpgo_debug_p2p_plan).
    exported[r] / needed[r]: lists of (node, pose) keys of every rank.  Returns (peers, send_keys, recv_keys) with
    peers = [(rank, send_off, send_cnt, recv_off, recv_cnt), ...]."""
    n = len(exported)
    def flat(lists):
        cnt = np.asarray([len(l) for l in lists], np.int32)
        nodes = np.asarray([k[0] for l in lists for k in l] or [0], np.int32)
        poses = np.asarray([k[1] for l in lists for k in l] or [0], np.int32)
        return cnt, nodes, poses
    ec, en, ep = flat(exported)
    nc, nn_, npz = flat(needed)
    sizes = np.zeros(3, np.int32)
    if lib().dpgo_debug_p2p_plan(rank, n, _ip(ec), _ip(en), _ip(ep), _ip(nc), _ip(nn_), _ip(npz), None, None, None, _ip(sizes)) != 0:
        raise ValueError("p2p_plan")
    peers = np.zeros(max(5 * int(sizes[0]), 1), np.int32)
    sk = np.zeros(max(2 * int(sizes[1]), 1), np.int32)
    rk = np.zeros(max(2 * int(sizes[2]), 1), np.int32)
    lib().dpgo_debug_p2p_plan(rank, n, _ip(ec), _ip(en), _ip(ep), _ip(nc), _ip(nn_), _ip(npz), _ip(peers), _ip(sk), _ip(rk), _ip(sizes))
    P = [tuple(int(v) for v in peers[5 * i:5 * i + 5]) for i in range(int(sizes[0]))]
    S = [(int(sk[2 * i]), int(sk[2 * i + 1])) for i in range(int(sizes[1]))]
    R = [(int(rk[2 * i]), int(rk[2 * i + 1])) for i in range(int(sizes[2]))]
    return P, S, R


class DChordalOptions(C.Structure):
    """DChordal::Options::reg_G + the driver's stage schedule (dist_pgo.cpp:205,274,344,383) + stage-0 length."""
    _fields_ = [("iters", C.c_int * 4), ("local_iters", C.c_int), ("reg_G", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_dchordal_options_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class Results(C.Structure):
    """Scalar part of DPGOResult (C++/DPGO/include/DPGO/DPGO_types.h:204-322)."""
    _fields_ = [
        ("updated", C.c_int), ("iters", C.c_int), ("gradFnorm", C.c_double), ("fobjE", C.c_double),
        ("Fk", C.c_double * 2), ("Gk", C.c_double), ("Gkh", C.c_double), ("fobj", C.c_double),
        ("f", C.c_double), ("gamma", C.c_double), ("s", C.c_double * 2),
        ("soft_restart_hits", C.c_int * 2), ("num_oscillations", C.c_int), ("refined", C.c_int),
        ("tnt_status", C.c_int), ("tnt_inner_iterations", C.c_int), ("restarts", C.c_int),
    ]


_lib = None
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int)

# every symbol of include/dpgo_amd.h: (restype, argtypes)
SYMBOLS = {
    "dpgo_options_default": (None, [C.POINTER(Options)]),
    "dpgo_options_driver": (None, [C.POINTER(Options), C.c_int, C.c_int]),
    "dpgo_read_g2o": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_graph_from_edges": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, _IP, _DP, _DP, _DP, _DP, C.c_int,
                                        C.POINTER(C.c_void_p)]),
    "dpgo_graph_free": (None, [C.c_void_p]),
    "dpgo_graph_info": (C.c_int, [C.c_void_p, _IP, _IP, _IP, _IP]),
    "dpgo_graph_edges": (C.c_int, [C.c_void_p, _IP, _IP, _DP, _DP, _DP, _DP]),
    "dpgo_graph_node_sizes": (C.c_int, [C.c_void_p, C.c_int, _IP, _IP, _IP, _IP]),
    "dpgo_graph_node_neighbours": (C.c_int, [C.c_void_p, C.c_int, _IP, _IP]),
    "dpgo_graph_node_offset": (C.c_int, [C.c_void_p, C.c_int]),
    "dpgo_graph_exchange_plan": (C.c_int, [C.c_void_p, _IP, C.c_int, _IP, _IP, _IP, _IP, _IP]),
    "dpgo_chordal_initialization": (C.c_int, [C.c_void_p, _DP, C.c_int]),
    "dpgo_graph_node_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _IP, _IP, _IP, _IP, _IP]),
    "dpgo_write_g2o": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_char_p]),
    "dpgo_group_evaluate": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP, C.c_int]),
    "dpgo_group_set_options": (C.c_int, [C.c_void_p, C.POINTER(Options)]),
    "dpgo_group_get_options": (C.c_int, [C.c_void_p, C.POINTER(Options)]),
    "dpgo_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dpgo_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "dpgo_comm_free": (None, [C.c_void_p]),
    "dpgo_comm_exchange": (C.c_int, [C.c_void_p]),
    "dpgo_comm_allreduce_sum": (C.c_int, [C.c_void_p, _DP, C.c_long]),
    "dpgo_comm_barrier": (C.c_int, [C.c_void_p]),
    "dpgo_comm_exchange_kind": (C.c_int, [C.c_void_p]),
    "dpgo_comm_bytes_sent": (C.c_long, [C.c_void_p]),
    "dpgo_comm_self_exchange": (C.c_int, [C.c_void_p]),
    "dpgo_comm_create_self": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "dpgo_comm_enable_timing": (C.c_int, [C.c_void_p]),
    "dpgo_comm_exchange_time": (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_long)]),
    "dpgo_debug_comm_p2p_self": (C.c_int, [C.c_void_p]),
    "dpgo_host_pack_sent": (C.c_int, [C.c_void_p, _IP, C.c_int, _DP, C.c_int, _DP]),
    "dpgo_host_unpack_recv": (C.c_int, [C.c_void_p, _IP, C.c_int, C.c_int, C.c_int, C.c_int, _IP, _IP, _IP, _DP, _DP,
                                        C.c_int]),
    "dpgo_dchordal_options_default": (None, [C.c_void_p]),
    "dpgo_group_dist_chordal_initialization": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, _DP, C.c_int, _DP, _IP]),
    "dpgo_group_create": (C.c_int, [C.c_void_p, _IP, C.c_int, C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_group_free": (None, [C.c_void_p]),
    "dpgo_group_initialize": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int]),
    "dpgo_group_initialize_global": (C.c_int, [C.c_void_p, _DP, C.c_int]),
    "dpgo_group_update": (C.c_int, [C.c_void_p, _IP, C.c_int]),
    "dpgo_group_iterate": (C.c_int, [C.c_void_p, _IP, C.c_int]),
    "dpgo_group_communicate_local": (C.c_int, [C.c_void_p]),
    "dpgo_group_step": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_message_sizes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _IP, _IP]),
    "dpgo_group_send": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _DP, C.c_int]),
    "dpgo_group_receive": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _DP, C.c_int]),
    "dpgo_group_set_collectives": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dpgo_group_star_initialize": (C.c_int, [C.c_void_p, _DP, C.c_int]),
    "dpgo_group_star_update": (C.c_int, [C.c_void_p]),
    "dpgo_group_star_iterate": (C.c_int, [C.c_void_p]),
    "dpgo_group_star_state": (C.c_int, [C.c_void_p, _DP, _DP, _DP, _IP]),
    "dpgo_group_num_sent": (C.c_int, [C.c_void_p]),
    "dpgo_group_sent_keys": (C.c_int, [C.c_void_p, _IP, _IP]),
    "dpgo_group_set_recv_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _IP, _IP, _IP]),
    "dpgo_group_pack_sent": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_unpack_recv": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_get_Xk": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int]),
    "dpgo_group_get_Xak": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int]),
    "dpgo_group_scatter_global": (C.c_int, [C.c_void_p, _DP, C.c_int]),
    "dpgo_group_results": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Results)]),
    "dpgo_group_node_id": (C.c_int, [C.c_void_p, C.c_int]),
    "dpgo_group_sync": (C.c_int, [C.c_void_p]),
    "dpgo_group_stream": (C.c_void_p, [C.c_void_p]),
    "dpgo_prof_enable": (C.c_int, [C.c_int]),
    "dpgo_prof_num_kinds": (C.c_int, []),
    "dpgo_prof_kind_name": (C.c_char_p, [C.c_int]),
    "dpgo_prof_collect": (C.c_int, [_DP, _DP, C.POINTER(C.c_long)]),
    "dpgo_prof_collect_operands": (C.c_int, [_DP]),
    "dpgo_group_solver_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), _IP, _IP]),
    "dpgo_group_graph_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "dpgo_debug_node_matrix": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Options), C.c_char_p, _IP, _IP, _DP]),
    "dpgo_debug_node_proximal": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Options), _DP, _DP, _DP]),
    "dpgo_debug_spd_solve": (C.c_int, [C.c_int, _IP, _IP, _DP, _DP, C.c_int, C.c_int]),
    "dpgo_debug_spd_stats": (C.c_int, [C.c_int, _IP, _IP, _DP, C.c_int, C.POINTER(C.c_long), _IP, _IP]),
    "dpgo_debug_spd_factor": (C.c_int, [C.c_int, _IP, _IP, _DP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_debug_spd_factor_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _IP, _DP, _IP, C.POINTER(C.c_longlong), _IP, _IP,
                                            _DP, _DP, _DP, _DP]),
    "dpgo_debug_spd_factor_free": (None, [C.c_void_p]),
    "dpgo_debug_spd_selinv": (C.c_int, [C.c_int, _IP, _IP, _DP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_debug_spd_selinv_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _IP, _DP, _IP, _IP, _IP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_spd_selinv_free": (None, [C.c_void_p]),
    "dpgo_debug_spd_vsolve": (C.c_int, [C.c_int, _IP, _IP, _DP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, _IP, _DP]),
    "dpgo_debug_spd_vsolve_chunk": (C.c_int, [C.c_int]),
    "dpgo_group_pair_covariance": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, _IP, C.c_int, _DP, _DP, _DP, _DP,
                                             C.c_void_p]),
    "dpgo_graph_pair_covariance_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, C.c_int,
                                                        C.c_longlong, _IP, C.c_int, _DP, _DP, _DP, _DP, C.c_void_p, C.c_void_p]),
    "dpgo_debug_pairs_vsolve_baseline": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, _DP]),
    "dpgo_debug_pairs_plan": (C.c_int, [C.c_int, C.c_int, _IP, C.c_int, _IP, _IP, _IP]),
    "dpgo_debug_pairs_gate": (C.c_int, [C.c_int, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_group_joint_marginal": (C.c_int, [C.c_void_p, _DP, C.c_int, _IP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, _DP, _DP,
                                            _DP, C.c_void_p]),
    "dpgo_graph_joint_marginal_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, _IP, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_longlong, _DP, _DP, _DP, C.c_void_p, C.c_void_p]),
    "dpgo_debug_marg_plan": (C.c_int, [C.c_int, C.c_int, _IP, C.c_int, _IP, _IP, _IP]),
    "dpgo_debug_marg_rel_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _DP, _DP, _DP]),
    "dpgo_debug_marg_rel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP]),
    "dpgo_debug_marg_dense": (C.c_int, [C.c_int, C.c_int, _DP, _DP, _DP, _DP, C.c_void_p]),
    "dpgo_group_candidate_set": (C.c_int, [C.c_void_p, _DP, C.c_int, _IP, C.c_int, _DP, C.c_int, C.c_int, C.c_double, C.c_int,
                                           C.c_longlong, _DP, _DP, _DP, _DP, _DP, _IP, _DP, _IP, C.c_void_p]),
    "dpgo_graph_candidate_set_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, _IP, C.c_int, _DP,
                                                      C.c_int, C.c_int, C.c_double, C.c_int, C.c_longlong, _DP, _DP, _DP, _DP, _DP,
                                                      _IP, _DP, _IP, C.c_void_p, C.c_void_p]),
    "dpgo_debug_cand_innov_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_cand_innov": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _IP, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_cand_select_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP, _IP, _DP, _DP, _IP]),
    "dpgo_debug_cand_select": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP, _IP, _DP, _DP, _IP]),
    "dpgo_group_sensitivity": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, _DP, C.c_int, C.c_int, _DP, _DP,
                                         C.c_void_p]),
    "dpgo_debug_sens_edge_host": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP]),
    "dpgo_group_edge_reliability": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, C.c_int, _IP, C.c_int, _DP,
                                              _DP, _DP, C.c_void_p]),
    "dpgo_graph_edge_reliability_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_longlong,
                                                         C.c_int, _IP, C.c_int, _DP, _DP, _DP, C.c_void_p, C.c_void_p]),
    "dpgo_debug_rely_edge_host": (C.c_int, [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_rely_edge": (C.c_int, [C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_spd_msolve": (C.c_int, [C.c_int, _IP, _IP, _DP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _DP, C.c_int,
                                        C.c_int, _DP, _IP, _DP]),
    "dpgo_debug_spd_solver_create": (C.c_int, [C.c_int, _IP, _IP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _IP, C.c_int,
                                               C.POINTER(C.c_void_p)]),
    "dpgo_debug_spd_solver_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), _IP, _IP, _IP, _IP, _IP, _IP]),
    "dpgo_debug_spd_solver_fine_root": (C.c_int, [C.c_void_p, C.c_ulonglong]),
    "dpgo_debug_spd_solver_run": (C.c_int, [C.c_void_p, C.c_ulonglong, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                            C.c_double, C.c_int, _DP, _DP]),
    "dpgo_debug_spd_solver_refactor": (C.c_int, [C.c_void_p, _DP]),
    "dpgo_debug_spd_solver_free": (None, [C.c_void_p]),
    "dpgo_debug_spd_panel_pack": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, _DP, C.c_int, _DP, C.c_longlong,
                                            C.POINTER(C.c_longlong)]),
    "dpgo_debug_p2p_plan": (C.c_int, [C.c_int, C.c_int, _IP, _IP, _IP, _IP, _IP, _IP, _IP, _IP, _IP, _IP]),
    "dpgo_group_debug_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, _DP, C.c_int, _DP, C.c_int]),
    "dpgo_group_debug_stpcg": (C.c_int, [C.c_void_p, _IP, C.c_int, _DP, C.c_int, _DP, C.c_int, C.c_double, _DP, C.c_int, _DP]),
    "dpgo_group_debug_seg_layout": (C.c_int, [C.c_void_p, _IP, _IP, _IP]),
    "dpgo_group_debug_inter_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_debug_inter_iterate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_debug_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _DP, _DP]),
    "dpgo_group_debug_edge_offsets": (C.c_int, [C.c_void_p, _IP]),
    "dpgo_group_debug_rescale": (C.c_int, [C.c_void_p, _DP, _DP, _IP, C.c_int, _IP, C.c_int, _IP, _DP, _DP, _IP]),
    "dpgo_group_debug_cg_scalars": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _DP, C.POINTER(C.c_ulonglong), _DP, _DP, _DP,
                                              C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), _DP, C.POINTER(C.c_ulonglong)]),
    "dpgo_group_debug_star_sums": (C.c_int, [C.c_void_p, _DP, C.c_uint, _DP, C.POINTER(C.c_ulonglong)]),
    "dpgo_group_debug_gated_update": (C.c_int, [C.c_void_p, C.c_ulonglong, _IP]),
    "dpgo_pcm_options_default": (None, [C.c_void_p]),
    "dpgo_pcm_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_pcm_free": (None, [C.c_void_p]),
    "dpgo_pcm_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _DP, C.c_int, C.c_void_p]),
    "dpgo_pcm_measurements": (C.c_int, [C.c_void_p, _IP]),
    "dpgo_pcm_adjacency": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_pcm_errors": (C.c_int, [C.c_void_p, _DP]),
    "dpgo_pcm_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dpgo_max_clique": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dpgo_graph_filter_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "dpgo_cert_options_default": (None, [C.c_void_p]),
    "dpgo_group_certify": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_void_p, _DP, C.c_int, C.c_void_p, _DP, C.c_int]),
    "dpgo_group_cert_lambda": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP]),
    "dpgo_group_cert_factor": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_double, C.c_longlong, C.c_void_p]),
    "dpgo_group_covariance": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, _IP, C.c_int, _DP, _DP, C.c_void_p]),
    "dpgo_group_cov_hessian": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, _IP, _IP, _DP, C.c_longlong, C.POINTER(C.c_longlong)]),
    "dpgo_graph_covariance_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_longlong,
                                                   _IP, C.c_int, _DP, _DP, C.c_void_p, C.c_void_p]),
    "dpgo_polish_options_default": (None, [C.c_void_p]),
    "dpgo_group_polish": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_void_p, C.c_longlong, _DP, C.c_int, _DP, C.c_int, C.c_void_p]),
    "dpgo_modes_options_default": (None, [C.c_void_p]),
    "dpgo_group_hessian_modes": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong, _DP, _DP, _DP, _DP, _DP,
                                           C.c_void_p]),
    "dpgo_debug_modes_init": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, _DP]),
    "dpgo_debug_modes_gram": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, _DP, _DP, _DP, _DP]),
    "dpgo_debug_modes_update": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_modes_ritz_host": (C.c_int, [C.c_int, _DP, _DP, _DP, _DP, _IP]),
    "dpgo_debug_modes_ritz": (C.c_int, [C.c_int, C.c_longlong, C.c_int, C.c_int, _DP, _DP, _DP, _DP, _IP]),
    "dpgo_group_robust_polish": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_longlong,
                                           _DP, C.c_int, _DP, C.c_int, C.c_void_p, C.c_void_p]),
    "dpgo_group_robust_covariance": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                               C.c_longlong, _IP, C.c_int, _DP, _DP, C.c_void_p]),
    "dpgo_group_robust_hessian": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _IP, _IP, _DP,
                                            C.c_longlong, C.POINTER(C.c_longlong), _DP, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_group_robust_matrix": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, _IP, _IP, _DP, C.c_longlong,
                                           C.POINTER(C.c_longlong)]),
    "dpgo_debug_robust_edge_host": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP, _DP]),
    "dpgo_graph_from_edges_info": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, _IP, _DP, _DP, _DP, _DP, _DP, C.c_int,
                                             C.POINTER(C.c_void_p)]),
    "dpgo_graph_edge_information": (C.c_int, [C.c_void_p, _DP, _IP]),
    "dpgo_group_ml_polish": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_void_p, C.c_longlong, _DP, C.c_int, _DP, C.c_int,
                                       C.c_void_p]),
    "dpgo_group_ml_covariance": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, _IP, C.c_int, _DP, _DP,
                                           C.c_void_p]),
    "dpgo_group_ml_edge_reliability": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, C.c_int, _IP, C.c_int,
                                                 _DP, _DP, _DP, C.c_void_p]),
    "dpgo_group_ml_pair_gate": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_longlong, _IP, C.c_int, _DP, _DP, _DP,
                                          _DP, _DP, _DP, C.c_void_p]),
    "dpgo_debug_ml_rely_edge_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_debug_ml_rely_edge": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_group_ml_hessian": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, _IP, _IP, _DP, C.c_longlong,
                                        C.POINTER(C.c_longlong), _DP, _DP]),
    "dpgo_group_ml_eval": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, _DP, C.POINTER(C.c_longlong), _DP, _DP, _DP, _DP, _DP]),
    "dpgo_group_debug_ml_hessian_guarded": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, C.c_double, _DP, _DP,
                                                      C.c_longlong]),
    "dpgo_debug_ml_edge_host": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(C.c_longlong)]),
    "dpgo_group_robust_sensitivity": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_longlong, _DP,
                                                C.c_int, C.c_int, _DP, _DP, _DP, C.c_void_p]),
    "dpgo_debug_robust_sens_edge_host": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP]),
    "dpgo_gnc_options_default": (None, [C.c_void_p]),
    "dpgo_group_gnc": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_void_p, _IP, C.c_longlong, _DP, C.c_int, _DP, _DP, C.c_int,
                                 C.c_void_p]),
    "dpgo_group_gnc_eval": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_double, _IP, _DP, _DP, _DP, _DP,
                                      _DP]),
    "dpgo_debug_gnc_weight_host": (C.c_int, [C.c_int, C.c_double, C.c_double, _DP, C.c_int, _DP, _DP]),
    "dpgo_group_ml_gnc": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_void_p, _IP, C.c_longlong, _DP, C.c_int, _DP, _DP,
                                    C.c_int, C.c_void_p]),
    "dpgo_group_ml_gnc_eval": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, C.c_double, _IP, _DP, C.c_int,
                                         _DP, _DP, _DP, _DP, _DP, _DP, _DP]),
    "dpgo_group_debug_ml_gnc_hessian": (C.c_int, [C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, _IP, _DP, _IP, _IP, _DP,
                                                  C.c_longlong, C.POINTER(C.c_longlong), _DP]),
    "dpgo_debug_ml_gnc_edge_host": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(C.c_longlong),
                                              C.POINTER(C.c_longlong)]),
    "dpgo_staircase_options_default": (None, [C.c_void_p]),
    "dpgo_group_staircase": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_void_p, C.c_longlong, _DP, C.c_int, _DP, C.c_int, _DP, C.c_int,
                                       C.c_void_p]),
    "dpgo_group_stair_eval": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP, _DP, C.c_int]),
    "dpgo_group_stair_hess": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, C.c_int, _DP, C.c_int]),
    "dpgo_group_stair_retract": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, C.c_int, _DP, C.c_int]),
    "dpgo_group_stair_round": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, _DP, _DP, C.c_int]),
    "dpgo_group_verify": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_void_p, C.c_longlong, _DP, C.c_int, C.c_void_p, _DP, C.c_int,
                                    C.c_void_p]),
    "dpgo_group_cert_matrix": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_double, _IP, _IP, _DP, C.c_longlong,
                                         C.POINTER(C.c_longlong)]),
    "dpgo_group_cert_apply": (C.c_int, [C.c_void_p, _DP, C.c_int, _DP, C.c_int, _DP, C.c_int]),
    "dpgo_debug_rayleigh_ritz": (C.c_int, [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _IP]),
    "dpgo_group_debug_cert_gram": (C.c_int, [C.c_void_p, _DP, _DP, _DP, _DP, _DP, _DP, _DP, C.c_int, _DP, _DP]),
    "dpgo_group_debug_cert_update": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dpgo_group_debug_cert_nbr_rows": (C.c_int, [C.c_void_p]),
    "dpgo_group_debug_cert_precon": (C.c_int, [C.c_void_p, _DP]),
    "dpgo_group_debug_cert_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "dpgo_group_debug_cert_trace_get": (C.c_int, [C.c_void_p, _DP, C.c_longlong, _IP, C.POINTER(C.c_longlong)]),
    "dpgo_edge_eval_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "dpgo_edge_eval_free": (None, [C.c_void_p]),
    "dpgo_edge_eval_run": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP, _DP, C.c_void_p]),
    "dpgo_edge_eval_kernel_ms": (C.c_int, [C.c_void_p, _DP]),
    "dpgo_debug_edge_eval_host": (C.c_int, [C.c_void_p, _DP, C.c_int, C.c_int, C.c_double, _DP, _DP, _DP, _DP, C.c_void_p]),
    "dpgo_graph_scale_edges": (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_void_p)]),
    "dpgo_graph_verify_reweighted": (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_longlong,
                                               C.c_void_p, C.c_void_p, C.c_void_p, _DP, C.c_int]),
}


def lib():
    """Load libdpgo_amd.so (built by dpgo_amd/csrc/Makefile).  Fails loudly if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("dpgo_amd: %s not found -- build it with __graft_entry__.build() "
                               "(make -C dpgo_amd/csrc); there is no fallback path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(_DP)


def _ip(a):
    return a.ctypes.data_as(_IP)


def _fcol(X):
    """Column-major float64 copy/view and its leading dimension."""
    X = np.asfortranarray(X, dtype=np.float64)
    return X, X.shape[0]


_LLP = C.POINTER(C.c_longlong)


def _dpn(a):
    """_dp of an optional array."""
    return None if a is None else _dp(a)


def _dof(d):
    """Tangent dimensions of a pose: d for the translation, d (d - 1) / 2 for the rotation."""
    return d + d * (d - 1) // 2


def _csr_args(A_csr, refactor_values=None):
    """(n, ptr, col, val, val2) of a scipy matrix as the CSR-taking hooks read it: CSR with sorted indices, int32 and float64;
    val2: refactor_values as float64, one value per stored entry of A, or None."""
    A = A_csr.tocsr()
    A.sort_indices()
    ptr, col = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    val = np.ascontiguousarray(A.data, np.float64)
    val2 = None
    if refactor_values is not None:
        val2 = np.ascontiguousarray(refactor_values, np.float64)
        if val2.shape != val.shape:
            raise ValueError("refactor_values must have one value per stored entry of A")
    return A.shape[0], ptr, col, val, val2


def _front_header(get, h):
    """The first of a front-by-front hook's two calls: (sizes (8), status (4), pivots (4)); the arrays come with the second."""
    sizes, status, piv = np.zeros(8, np.int64), np.zeros(4, np.int32), np.zeros(4)
    get(h, sizes.ctypes.data_as(_LLP), _ip(status), _dp(piv), *[None] * 8)
    return sizes, status, piv


def _per_front(w, u, piv_idx, upd_idx):
    """The flat pivot and update row lists of a factor, cut into one array per front (widths w, update rows u)."""
    pp, up = np.concatenate([[0], np.cumsum(w)]), np.concatenate([[0], np.cumsum(u)])
    return ([piv_idx[pp[s]:pp[s + 1]].copy() for s in range(len(w))], [upd_idx[up[s]:up[s + 1]].copy() for s in range(len(w))])


def _csr_out(n, what, call, fetch=None):
    """A CSR matrix of n rows read back from the library: call(None, None, None, 0, nnz) asks for the number of entries,
    fetch (default: call again) fills (ptr, col, val, cap, nnz).  Returns (ptr, col, val)."""
    nnz = C.c_longlong(0)
    if call(None, None, None, 0, C.byref(nnz)) != 0:
        raise RuntimeError("%s failed" % what)
    ptr, col, val = np.zeros(n + 1, np.int32), np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
    if (fetch or call)(_ip(ptr), _ip(col), _dp(val), nnz.value, C.byref(nnz)) != 0:
        raise RuntimeError("%s failed" % what)
    return ptr, col, val


def _cert_args(X, what, eta, tau, max_iters, precondition, stop_on_negative, refresh_every, seed, V0=None):
    """What certify, verify and verify_reweighted hand the library: (CertOptions, V0 or None, its pointer, its ld); V0 must
    have the shape of X."""
    o = CertOptions(eta=eta, tau=tau, max_iters=int(max_iters), precondition=int(bool(precondition)),
                    stop_on_negative=int(bool(stop_on_negative)), refresh_every=int(refresh_every), seed=int(seed))
    if V0 is None:
        return o, None, None, 0
    V0 = np.asarray(V0)
    if V0.shape != X.shape:
        raise ValueError("%s: V0 must have the shape of X, %r" % (what, X.shape))
    V0, ldv0 = _fcol(V0)
    return o, V0, _dp(V0), ldv0


def _pairs_arg(pairs, num_poses, dof):
    """The pairs of a covariance call and the arrays it fills: (marg (N, dof, dof), cross (npairs, dof, dof), the four
    arguments pairs, npairs, marginals, cross of the C call).  pairs: None or (npairs, 2) global poses."""
    P = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
    marg, cross = np.zeros((num_poses, dof, dof)), np.zeros((len(P), dof, dof))
    return marg, cross, (_ip(P) if len(P) else None, len(P), _dp(marg), _dp(cross) if len(P) else None)


def _marg_arg(d, keep, base, want_info):
    """The arrays of a joint_marginal call: (cov, info, logdet, order, (keep pointer, K, base as the C ABI takes it)); the
    arrays have the size of a VALID call -- the library checks the list itself."""
    K = np.ascontiguousarray(np.asarray(keep).reshape(-1), np.int32)
    if len(K) < 1:
        raise ValueError("joint_marginal: keep is empty")
    dof = _dof(d)
    b = -1 if base is None else int(base)
    if b < -1:
        raise ValueError("joint_marginal: base is negative")
    order = K.copy() if b < 0 else K[K != b].copy()
    n = max(dof * (len(K) - (0 if b < 0 else 1)), 1)
    cov, info, logdet = np.zeros((n, n)), np.zeros((n, n)), np.zeros(1)
    return cov, info, logdet, order, (_ip(K), len(K), b, K)


def _cand_pack(d, m, candidates):
    """(m, d^2 + d + 2) from a tuple (R, t, kappa, tau) (pack_candidates) or an array already in that layout."""
    if isinstance(candidates, tuple):
        return pack_candidates(d, m, *candidates)
    cand = np.ascontiguousarray(candidates, np.float64).reshape(m, -1)
    if cand.shape[1] != d * d + d + 2:
        raise ValueError("candidates: %d values per candidate, not d^2 + d + 2" % cand.shape[1])
    return cand


def _cand_arg(d, pairs, candidates, budget, want_joint, want_cov):
    """The arrays of a candidate_set call, sized for a VALID call -- the library checks the pairs and weights itself: (a dict of
    the arrays, the arguments pairs, ncand, candidates and, after the scalars the caller puts between, cov ... poses)."""
    P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
    m, budget = len(P), int(budget)
    if m < 1:
        raise ValueError("candidate_set: no candidates")
    if budget < 0:
        raise ValueError("candidate_set: the budget is negative")
    n = _dof(d) * m
    a = {"cand": _cand_pack(d, m, candidates), "pairs": P, "cov": np.zeros((n, n)) if want_cov else None,
         "S": np.zeros((n, n)) if want_cov else None, "residual": np.zeros(n), "info": np.zeros((n, n)) if want_joint else None,
         "scalars": np.zeros(5), "selected": np.full(max(budget, 1), -1, np.int32), "steps": np.zeros((max(budget, 1), 4)),
         "poses": np.zeros(2 * m, np.int32), "budget": budget}
    head = (_ip(P), m, _dp(a["cand"]))
    tail = (_dpn(a["cov"]), _dpn(a["S"]), _dp(a["residual"]), _dpn(a["info"]), _dp(a["scalars"]), _ip(a["selected"]), _dp(a["steps"]),
            _ip(a["poses"]))
    return a, head, tail


def _pair_cov_arg(d, pairs, candidates):
    """The pairs and candidates of a pair_covariance call and the arrays it fills: (gated, joint, rel, gate, the six
    arguments pairs, npairs, candidates, joint, rel, gate of the C call)."""
    dof = _dof(d)
    P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
    cand = None if candidates is None else pack_candidates(d, len(P), *candidates)
    joint, rel, gate = np.zeros((len(P), 3, dof, dof)), np.zeros((len(P), dof, dof)), np.zeros((len(P), 2 + dof))
    return cand is not None, joint, rel, gate, (_ip(P) if len(P) else None, len(P), _dpn(cand), _dp(joint), _dp(rel), _dp(gate))


def _polish_arg(X, anchor, opts):
    """What polish and robust_polish hand the library: (X, ld, PolishOptions, Xout starting as X, the log array)."""
    X, ld = _fcol(X)
    o = PolishOptions(anchor=int(anchor), **opts)
    return X, ld, o, np.array(X, order="F"), np.zeros((max(int(o.max_steps), 0) + 1, 5))


def _polish_log(log, r):
    """The rows of the log a polish wrote: one per iteration, none for POLISH_SKIPPED."""
    return log[:0 if r.outcome == POLISH_SKIPPED else min(len(log), r.steps + 1)].copy()


class Graph:
    """Result of DPGO::read_g2o: measurements partitioned over num_nodes."""

    def __init__(self, handle):
        self._h = handle
        d, n, k, m = (C.c_int() for _ in range(4))
        lib().dpgo_graph_info(self._h, C.byref(d), C.byref(n), C.byref(k), C.byref(m))
        self.d, self.num_poses, self.num_nodes, self.num_edges = d.value, n.value, k.value, m.value

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dpgo_graph_free(self._h)
            self._h = None

    def edges(self):
        d, m = self.d, self.num_edges
        I, J = np.empty(m, np.int32), np.empty(m, np.int32)
        R, t = np.empty((m, d, d)), np.empty((m, d))
        kap, tau = np.empty(m), np.empty(m)
        lib().dpgo_graph_edges(self._h, _ip(I), _ip(J), _dp(R), _dp(t), _dp(kap), _dp(tau))
        return I, J, R, t, kap, tau

    def edge_information(self):
        """Every edge's information matrix (dpgo_graph_edge_information): (Omega (m, dof, dof), has).  has False: the graph
        keeps none of its own (it was built from arrays without them) and Omega is Omega_iso = diag(tau I_d, 2 kappa I)."""
        dof = _dof(self.d)
        om, has = np.zeros((self.num_edges, dof, dof)), np.zeros(1, np.int32)
        if lib().dpgo_graph_edge_information(self._h, _dp(om), _ip(has)) != 0:
            raise ValueError("dpgo_graph_edge_information failed")
        return om, bool(has[0])

    def node_sizes(self, node):
        v = [C.c_int() for _ in range(4)]
        if lib().dpgo_graph_node_sizes(self._h, node, *[C.byref(x) for x in v]) != 0:
            raise ValueError("node %d" % node)
        return tuple(x.value for x in v)   # n0, n1, m0, m1

    def node_neighbours(self, node):
        n1 = self.node_sizes(node)[1]
        a, b = np.empty(n1, np.int32), np.empty(n1, np.int32)
        lib().dpgo_graph_node_neighbours(self._h, node, _ip(a), _ip(b))
        return a, b

    def node_offset(self, node):
        return lib().dpgo_graph_node_offset(self._h, node)

    def exchange_plan(self, node_ids):
        """(sent (node, pose) keys, recv (node, pose) keys) of a group hosting node_ids (host only)."""
        ids = np.asarray(list(node_ids), np.int32)
        cnt = np.zeros(2, np.int32)
        if lib().dpgo_graph_exchange_plan(self._h, _ip(ids), len(ids), None, None, None, None, _ip(cnt)) != 0:
            raise ValueError("exchange_plan")
        sn, sp_, rn, rp = (np.empty(c, np.int32) for c in (cnt[0], cnt[0], cnt[1], cnt[1]))
        lib().dpgo_graph_exchange_plan(self._h, _ip(ids), len(ids), _ip(sn), _ip(sp_), _ip(rn), _ip(rp), _ip(cnt))
        return (sn, sp_), (rn, rp)

    def node_maps(self, node, which):
        """DPGOProblem::index() / sent() / recv() (which = "index" | "sent" | "recv"):
        list of ((node, pose), (block, k)) in map order."""
        w = {"index": 0, "sent": 1, "recv": 2}[which]
        cnt = C.c_int()
        if lib().dpgo_graph_node_maps(self._h, node, w, None, None, None, None, C.byref(cnt)) != 0:
            raise ValueError("node_maps")
        a, b, c, d = (np.empty(cnt.value, np.int32) for _ in range(4))
        lib().dpgo_graph_node_maps(self._h, node, w, _ip(a), _ip(b), _ip(c), _ip(d), C.byref(cnt))
        return [((int(a[i]), int(b[i])), (int(c[i]), int(d[i]))) for i in range(cnt.value)]

    def write_g2o(self, filename, X=None):
        """VERTEX_* lines from X (optional) + EDGE_* lines; returns 0 / -1."""
        if X is None:
            return lib().dpgo_write_g2o(self._h, None, 0, os.fsencode(filename))
        X, ld = _fcol(X)
        return lib().dpgo_write_g2o(self._h, _dp(X), ld, os.fsencode(filename))

    def host_pack_sent(self, node_ids, X):
        """Records of the poses a group hosting node_ids exports (key order), from a global X: what
        dpgo_group_pack_sent puts into the device buffer (host version, no GPU)."""
        ids = np.asarray(list(node_ids), np.int32)
        (sn, _), _ = self.exchange_plan(ids)
        X, ld = _fcol(X)
        buf = np.zeros(max(len(sn), 1) * (self.d + 1) * self.d)
        n = lib().dpgo_host_pack_sent(self._h, _ip(ids), len(ids), _dp(X), ld, _dp(buf))
        if n < 0:
            raise RuntimeError("dpgo_host_pack_sent failed")
        return buf[:n * (self.d + 1) * self.d]

    def host_unpack_recv(self, node_ids, node, stride, keys_per_rank, gathered, Z):
        """Fill the neighbour rows of node's Z ((d+1)(n0+n1) x d, F order) from the gathered buffers (host version
        of dpgo_group_unpack_recv); returns the number of poses written."""
        ids = np.asarray(list(node_ids), np.int32)
        counts = np.asarray([len(k[0]) for k in keys_per_rank], np.int32)
        nodes = np.ascontiguousarray(np.concatenate([np.asarray(k[0], np.int32) for k in keys_per_rank]), np.int32)
        poses = np.ascontiguousarray(np.concatenate([np.asarray(k[1], np.int32) for k in keys_per_rank]), np.int32)
        gathered = np.ascontiguousarray(gathered, np.float64)
        assert Z.flags.f_contiguous
        n = lib().dpgo_host_unpack_recv(self._h, _ip(ids), len(ids), int(node), len(counts), int(stride), _ip(counts),
                                        _ip(nodes), _ip(poses), _dp(gathered), _dp(Z), Z.shape[0])
        if n < 0:
            raise RuntimeError("dpgo_host_unpack_recv failed")
        return n

    def chordal_initialization(self):
        """Centralised chordal init (dist_pgo.cpp:416-444): X, (d+1)N x d, reference layout."""
        X = np.zeros(((self.d + 1) * self.num_poses, self.d), order="F")
        if lib().dpgo_chordal_initialization(self._h, _dp(X), X.shape[0]) != 0:
            raise RuntimeError("chordal initialisation failed")
        return X

    def node_matrix(self, node, opt, name):
        """Assembled operator in the reference's row order, as a scipy COO matrix (test hook)."""
        import scipy.sparse as sp
        cnt = lib().dpgo_debug_node_matrix(self._h, node, C.byref(opt), name.encode(), None, None, None)
        if cnt < 0:
            raise ValueError(name)
        r, c, v = np.empty(cnt, np.int32), np.empty(cnt, np.int32), np.empty(cnt)
        lib().dpgo_debug_node_matrix(self._h, node, C.byref(opt), name.encode(), _ip(r), _ip(c), _dp(v))
        n0, n1, _, _ = self.node_sizes(node)
        D1 = self.d + 1
        shape = {"G": (D1 * n0, D1 * n0), "D": (D1 * n0, D1 * n0), "S": (D1 * n0, D1 * (n0 + n1))}.get(
            name, (D1 * (n0 + n1), D1 * (n0 + n1)))
        return sp.coo_matrix((v, (r, c)), shape=shape).tocsr()

    def filter_edges(self, keep):
        """The same poses and partition with only the edges where keep (length num_edges) is true, in order
        (dpgo_graph_filter_edges): how the closures PCM rejected are dropped before building groups."""
        keep = np.ascontiguousarray(np.asarray(keep, bool).astype(np.uint8))
        if keep.shape != (self.num_edges,):
            raise ValueError("keep must have one entry per edge (%d)" % self.num_edges)
        h = C.c_void_p()
        if lib().dpgo_graph_filter_edges(self._h, keep.ctypes.data_as(C.c_void_p), C.byref(h)) != 0:
            raise ValueError("filter_edges failed (no edge kept?)")
        return Graph(h)

    def scale_edges(self, w):
        """The same poses, partition, R, t and edge order with kappa_e, tau_e multiplied by w[e] (dpgo_graph_scale_edges):
        the graph of the re-weighted problem.  w[e] = 0 is legal (the edge stays, with zero values); a negative or
        non-finite weight raises ValueError."""
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.num_edges,):
            raise ValueError("w must have one entry per edge (%d)" % self.num_edges)
        h = C.c_void_p()
        if lib().dpgo_graph_scale_edges(self._h, _dp(w), C.byref(h)) != 0:
            raise ValueError("scale_edges failed (a negative or non-finite weight)")
        return Graph(h)

    def node_proximal(self, node, opt):
        n0 = self.node_sizes(node)[0]
        d = self.d
        T, N, V = np.empty(n0), np.empty((n0, d)), np.empty((n0, d, d))
        lib().dpgo_debug_node_proximal(self._h, node, C.byref(opt), _dp(T), _dp(N), _dp(V))
        return T, N, V


def read_g2o(filename, num_nodes):
    """DPGO::read_g2o (C++/DPGO/src/DPGO_utils.cpp:140-202)."""
    h = C.c_void_p()
    if lib().dpgo_read_g2o(os.fsencode(filename), int(num_nodes), C.byref(h)) != 0:
        raise IOError("read_g2o failed for %s" % filename)
    return Graph(h)


def graph_from_edges(d, num_poses, I, J, R, t, kappa, tau, num_nodes, info=None):
    """The graph of measurements in memory.  info (optional, (m, dof, dof)): every edge's full information matrix, which the
    graph then keeps for the maximum-likelihood refinement (dpgo_graph_from_edges_info); kappa and tau stay the caller's."""
    I, J = np.ascontiguousarray(I, np.int32), np.ascontiguousarray(J, np.int32)
    R, t = np.ascontiguousarray(R, np.float64), np.ascontiguousarray(t, np.float64)
    kappa, tau = np.ascontiguousarray(kappa, np.float64), np.ascontiguousarray(tau, np.float64)
    h = C.c_void_p()
    if info is None:
        rc = lib().dpgo_graph_from_edges(d, num_poses, len(I), _ip(I), _ip(J), _dp(R), _dp(t), _dp(kappa), _dp(tau),
                                         int(num_nodes), C.byref(h))
    else:
        info = np.ascontiguousarray(info, np.float64)
        if info.shape != (len(I), _dof(d), _dof(d)):
            raise ValueError("graph_from_edges: info must be (m, dof, dof)")
        rc = lib().dpgo_graph_from_edges_info(d, num_poses, len(I), _ip(I), _ip(J), _dp(R), _dp(t), _dp(kappa), _dp(tau),
                                              _dp(info), int(num_nodes), C.byref(h))
    if rc != 0:
        raise ValueError("graph_from_edges failed")
    return Graph(h)


Graph.from_edges = staticmethod(graph_from_edges)


def spd_solve_host(A_csr, B, leaf=32):
    """Host multifrontal factor + solve (test hook for the solver set-up path)."""
    n, ptr, col, val, _ = _csr_args(A_csr)
    X = np.ascontiguousarray(B, np.float64).copy()
    if X.ndim == 1:
        X = X[:, None]
    if lib().dpgo_debug_spd_solve(n, _ip(ptr), _ip(col), _dp(val), _dp(X), X.shape[1], leaf) != 0:
        raise RuntimeError("spd solve failed")
    return X


def prof_enable(on):
    lib().dpgo_prof_enable(int(bool(on)))


def prof_collect():
    """{kernel family: (total_ms, algorithmic_bytes, launches)} since prof_enable(True)."""
    n = lib().dpgo_prof_num_kinds()
    ms, by, cnt = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    lib().dpgo_prof_collect(_dp(ms), _dp(by), cnt.ctypes.data_as(C.POINTER(C.c_long)))
    return {lib().dpgo_prof_kind_name(k).decode(): (float(ms[k]), float(by[k]), int(cnt[k])) for k in range(n)}


def prof_collect_operands():
    """{kernel family: bytes of every operand its launches moved, counted one by one} -- non-zero for the fused passes
    (k_inter, k_proximal), whose duties SURVEY 8(d)'s per-unit formula does not price."""
    n = lib().dpgo_prof_num_kinds()
    ob = np.zeros(n)
    lib().dpgo_prof_collect_operands(_dp(ob))
    return {lib().dpgo_prof_kind_name(k).decode(): float(ob[k]) for k in range(n)}


def spd_stats(A_csr, leaf):
    n, ptr, col, val, _ = _csr_args(A_csr)
    nnz, lv, mf = C.c_long(), C.c_int(), C.c_int()
    if lib().dpgo_debug_spd_stats(n, _ip(ptr), _ip(col), _dp(val), leaf, C.byref(nnz), C.byref(lv), C.byref(mf)) != 0:
        raise RuntimeError("spd_stats failed")
    return nnz.value, lv.value, mf.value


def spd_factor_debug(A_csr, leaf, collapse=1, block=1, factor_only=False, refactor_values=None):
    """The multifrontal factor of a CSR matrix, front by front (test hook, dpgo_debug_spd_factor).

    It bypasses nothing: spd_factor(A, F, leaf, collapse, block) runs as a group calls it (quiet), with the numeric phase
    on the device where there is one and on the host otherwise or under DPGO_SPD_HOST_FACTOR=1.  refactor_values: a second
    value array in the order of A.tocsr() with sorted indices, factored afterwards through the kept numeric context
    (keep_device + keep_numeric, spd_refactor_device -- the path of a Dynamic rescale and of the certificate).
    factor_only: the certificate's route (spd_symbolic, spd_prepare_device, spd_refactor_device); verdicts and pivots only.

    Returns a dict: status (0 factored, 1 not positive definite), fail_front, pivot_min, pivot_max, on_device, nfronts,
    the per-front arrays w, u, parent, height, ldw, ldm, w_off, wt_off, the lists piv_idx / upd_idx (one array per front),
    W / WT (flat, as SpdFactor holds them; None when the factorisation failed or factor_only), and with refactor_values
    status2, fail_front2, pivot_min2, pivot_max2, W2, WT2."""
    n, ptr, col, val, val2 = _csr_args(A_csr, refactor_values)
    h = C.c_void_p()
    if lib().dpgo_debug_spd_factor(n, _ip(ptr), _ip(col), _dp(val), _dpn(val2), int(leaf), int(collapse), int(block),
                                   int(bool(factor_only)), C.byref(h)) != 0:
        raise RuntimeError("spd_factor_debug failed")
    try:
        get = lib().dpgo_debug_spd_factor_get
        sizes, status, piv = _front_header(get, h)
        nt = int(sizes[0])
        fronts = np.zeros((nt, 6), np.int32)
        offs = np.zeros((nt, 2), np.int64)
        piv_idx = np.zeros(n, np.int32)
        upd_idx = np.zeros(max(int(sizes[1]), 1), np.int32)
        W = np.zeros(int(sizes[2])) if sizes[4] else None
        WT = np.zeros(int(sizes[3])) if sizes[4] else None
        W2 = np.zeros(int(sizes[2])) if sizes[5] else None
        WT2 = np.zeros(int(sizes[3])) if sizes[5] else None
        opt = lambda a: None if a is None or a.size == 0 else _dp(a)
        get(h, None, None, None, _ip(fronts), offs.ctypes.data_as(_LLP), _ip(piv_idx), _ip(upd_idx), opt(W), opt(WT), opt(W2),
            opt(WT2))
    finally:
        lib().dpgo_debug_spd_factor_free(h)
    w, u = fronts[:, 0].copy(), fronts[:, 1].copy()
    piv_lists, upd_lists = _per_front(w, u, piv_idx, upd_idx)
    out = {"status": int(status[0]), "fail_front": int(status[1]), "pivot_min": float(piv[0]), "pivot_max": float(piv[1]),
           "on_device": bool(sizes[7]), "nfronts": nt, "w": w, "u": u, "parent": fronts[:, 2].copy(),
           "height": fronts[:, 3].copy(), "ldw": fronts[:, 4].copy(), "ldm": fronts[:, 5].copy(), "w_off": offs[:, 0].copy(),
           "wt_off": offs[:, 1].copy(), "piv_idx": piv_lists, "upd_idx": upd_lists, "W": W, "WT": WT}
    if sizes[6]:
        out.update(status2=int(status[2]), fail_front2=int(status[3]), pivot_min2=float(piv[2]), pivot_max2=float(piv[3]),
                   W2=W2, WT2=WT2)
    return out


def spd_selinv_debug(A_csr, leaf, collapse=1, block=1, host=False, refactor_values=None):
    """Selected inversion of an SPD CSR matrix, front by front (test hook, dpgo_debug_spd_selinv): the entries of A^-1 inside
    the factor's pattern, from spd_selinv_device where there is a HIP device and host is not asked for, else from
    spd_selinv_host.  refactor_values: a second value array in the order of A.tocsr() with sorted indices, factored through
    the kept numeric context and inverted afterwards.

    Returns a dict: status / selinv_status (0; 1: not positive definite, and then nothing was inverted), pivot_min,
    pivot_max, on_device, nfronts, w, u, parent, depth, piv_idx / upd_idx (one array per front), sigma (a list: per front
    the (w + u) x (w + u) block of A^-1 on [pivots; update rows], None when not inverted), sigma_again (a second call's),
    W_before / W_after (the factor's W ahead of the inversion and from a factorisation of the same values behind it), and
    with refactor_values status2, selinv_status2, pivot_min2, pivot_max2, sigma2."""
    n, ptr, col, val, val2 = _csr_args(A_csr, refactor_values)
    h = C.c_void_p()
    if lib().dpgo_debug_spd_selinv(n, _ip(ptr), _ip(col), _dp(val), _dpn(val2), int(leaf), int(collapse), int(block),
                                   int(bool(host)), C.byref(h)) != 0:
        raise RuntimeError("spd_selinv_debug failed")
    try:
        get = lib().dpgo_debug_spd_selinv_get
        sizes, status, piv = _front_header(get, h)
        nt = int(sizes[0])
        fronts = np.zeros((nt, 4), np.int32)
        piv_idx = np.zeros(n, np.int32)
        upd_idx = np.zeros(max(int(sizes[1]), 1), np.int32)
        flat = [np.zeros(int(sizes[k])) if sizes[k] else None for k in (3, 4, 5, 6, 6)]
        get(h, None, None, None, _ip(fronts), _ip(piv_idx), _ip(upd_idx), *[_dpn(a) for a in flat])
    finally:
        lib().dpgo_debug_spd_selinv_free(h)
    w, u = fronts[:, 0].copy(), fronts[:, 1].copy()
    piv_lists, upd_lists = _per_front(w, u, piv_idx, upd_idx)
    m = (w + u).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(m * m)])
    blocks = lambda a: None if a is None else [a[so[s]:so[s + 1]].reshape(m[s], m[s]) for s in range(nt)]
    out = {"status": int(status[0]), "selinv_status": int(status[1]), "pivot_min": float(piv[0]), "pivot_max": float(piv[1]),
           "on_device": bool(sizes[7]), "nfronts": nt, "w": w, "u": u, "parent": fronts[:, 2].copy(), "depth": fronts[:, 3].copy(),
           "piv_idx": piv_lists, "upd_idx": upd_lists, "sigma": blocks(flat[0]), "sigma_again": blocks(flat[1]),
           "W_before": flat[3], "W_after": flat[4]}
    if refactor_values is not None:
        out.update(status2=int(status[2]), selinv_status2=int(status[3]), pivot_min2=float(piv[2]), pivot_max2=float(piv[3]),
                   sigma2=blocks(flat[2]))
    return out


def spd_vsolve_debug(A_csr, rhs, leaf, collapse=1, block=1, host=False, refactor_values=None, chunk=None):
    """A^-1 rhs for one plain vector (test hook, dpgo_debug_spd_vsolve): spd_factor, then spd_vsolve_device on the factor as the
    numeric phase leaves it where there is a HIP device and host is not asked for, else spd_solve_host.  refactor_values: a
    second value array in the order of A.tocsr() with sorted indices, factored through the kept numeric context and solved
    with afterwards.  chunk: for the length of the call, the entries of a front's input vector the device stages at a time
    (dpgo_debug_spd_vsolve_chunk; default 2048).

    Returns a dict: status (0; 1: not positive definite, and then nothing was solved), on_device, pivot_min, pivot_max, out (the
    solution, None when not solved), out_again (a second call's), raw (the 3 n doubles the hook was handed, filled with `fill`
    first -- what it did not write is still there), and with refactor_values status2, pivot_min2, pivot_max2, out2."""
    n = A_csr.shape[0]
    b = np.ascontiguousarray(rhs, np.float64)
    if b.shape != (n,):
        raise ValueError("rhs must have one entry per unknown")
    n, ptr, col, val, val2 = _csr_args(A_csr, refactor_values)
    raw = np.full(3 * n, VSOLVE_FILL)
    status = np.zeros(2, np.int32)
    piv = np.zeros(4)
    before = lib().dpgo_debug_spd_vsolve_chunk(int(chunk)) if chunk is not None else None
    try:
        rc = lib().dpgo_debug_spd_vsolve(n, _ip(ptr), _ip(col), _dp(val), _dpn(val2), int(leaf), int(collapse), int(block),
                                         int(bool(host)), _dp(b), _dp(raw), _ip(status), _dp(piv))
    finally:
        if before is not None:
            lib().dpgo_debug_spd_vsolve_chunk(before)
    if rc < 0:
        raise RuntimeError("spd_vsolve_debug failed")
    ok = status[0] == 0
    out = {"status": int(status[0]), "on_device": rc == 1, "pivot_min": float(piv[0]), "pivot_max": float(piv[1]),
           "out": raw[:n].copy() if ok else None, "out_again": raw[n:2 * n].copy() if ok else None, "raw": raw}
    if refactor_values is not None:
        out.update(status2=int(status[1]), pivot_min2=float(piv[2]), pivot_max2=float(piv[3]),
                   out2=raw[2 * n:].copy() if status[1] == 0 else None)
    return out


# what spd_vsolve_debug fills its output with before the call: a quiet NaN with a payload (tests/solve_restatement.py: SENT_OUT)
VSOLVE_FILL = np.array([0x7ff8_0000_beef_0002], np.uint64).view(np.float64)[0]


def spd_msolve_debug(A_csr, rhs, leaf, collapse=1, block=1, host=False, refactor_values=None, chunk=None, ldx=None):
    """A^-1 rhs for a block of plain vectors, rhs n x k (test hook, dpgo_debug_spd_msolve): spd_factor, then spd_msolve_device
    on the factor as the numeric phase leaves it where there is a HIP device and host is not asked for, else
    spd_solve_host(F, X, k).  refactor_values: as for spd_vsolve_debug.  chunk: for the length of the call, the rows of a
    front's input block the device stages at a time (spd_msolve_chunk; default 32).  ldx >= k: the row length of the array
    the solve works in (default k).

    Returns a dict: status (0; 1: not positive definite, and then nothing was solved), on_device, pivot_min, pivot_max, out (the
    solution n x k, None when not solved), out_again (a second call's), raw (3 x n x ldx: the arrays the hook was handed,
    filled with VSOLVE_FILL first -- what it did not write is still there, the columns k ... ldx on the device included), and
    with refactor_values status2, pivot_min2, pivot_max2, out2."""
    n = A_csr.shape[0]
    b = np.ascontiguousarray(rhs, np.float64)
    if b.ndim != 2 or b.shape[0] != n or b.shape[1] < 1:
        raise ValueError("rhs must be n x k with k >= 1")
    k = b.shape[1]
    ldx = k if ldx is None else int(ldx)
    if ldx < k:
        raise ValueError("ldx must be at least k")
    n, ptr, col, val, val2 = _csr_args(A_csr, refactor_values)
    raw = np.full((3, n, ldx), VSOLVE_FILL)
    status = np.zeros(2, np.int32)
    piv = np.zeros(4)
    rc = lib().dpgo_debug_spd_msolve(n, _ip(ptr), _ip(col), _dp(val), _dpn(val2), int(leaf), int(collapse), int(block),
                                     int(bool(host)), 0 if chunk is None else int(chunk), _dp(b), k, ldx, _dp(raw), _ip(status),
                                     _dp(piv))
    if rc < 0:
        raise RuntimeError("spd_msolve_debug failed")
    ok = status[0] == 0
    out = {"status": int(status[0]), "on_device": rc == 1, "pivot_min": float(piv[0]), "pivot_max": float(piv[1]),
           "out": raw[0, :, :k].copy() if ok else None, "out_again": raw[1, :, :k].copy() if ok else None, "raw": raw}
    if refactor_values is not None:
        out.update(status2=int(status[1]), pivot_min2=float(piv[2]), pivot_max2=float(piv[3]),
                   out2=raw[2, :, :k].copy() if status[1] == 0 else None)
    return out


class SpdSolverDebug:
    """The device multifrontal solve on a given CSR matrix (test hook, dpgo_debug_spd_solver_*): spd_factor and
    SpdSolverDev::upload(dof, d, node_of_unknown) as a group runs them for G_tt (dof 1) and G_RR + lambda I (dof d), then
    spd_run.  Raises RuntimeError("no HIP device") without a GPU.

    plan()      what upload() decided: fused_root, root_sym, root_rows, root_fine_rows, root_fine_below, stream_once, the
                lists fwd / bwd and the entries root, root_fine, root_rows of dicts (rows, nwide, nnarrow, wcount, ncount --
                the last two per local node), and the front table w, u, parent, height, piv_idx, upd_idx
    run(...)    out <- scale * A^-1 in on the unknowns of the live nodes; returns the out array ((d + 1) d doubles per
                record), or None where spd_run itself refuses (in place with fused roots)
    refactor()  new values through the kept numeric context, then repack() (keep_numeric=True only)"""

    def __init__(self, A_csr, leaf, collapse=1, block=1, d=3, dof=1, node_of_unknown=None, keep_numeric=False):
        n, ptr, col, val, _ = _csr_args(A_csr)
        node = np.zeros(n, np.int32) if node_of_unknown is None else np.ascontiguousarray(node_of_unknown, np.int32)
        if node.shape != (n,):
            raise ValueError("node_of_unknown must have one entry per unknown")
        self._h = C.c_void_p()
        self.n, self.d, self.dof, self.nval = n, int(d), int(dof), len(val)
        rc = lib().dpgo_debug_spd_solver_create(n, _ip(ptr), _ip(col), _dp(val), int(leaf), int(collapse), int(block), int(d),
                                                int(dof), _ip(node), int(bool(keep_numeric)), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise RuntimeError("no HIP device" if rc == -2 else "dpgo_debug_spd_solver_create failed")
        self.records = (n + self.dof - 1) // self.dof
        self.shape = (self.records * (self.d + 1), self.d)

    def close(self):
        if getattr(self, "_h", None):
            lib().dpgo_debug_spd_solver_free(self._h)
            self._h = None

    __del__ = close

    def plan(self):
        get = lib().dpgo_debug_spd_solver_plan
        sizes = np.zeros(8, np.int64)
        flags = np.zeros(8, np.int32)
        get(self._h, sizes.ctypes.data_as(_LLP), _ip(flags), None, None, None, None, None)
        nt, nupd, nf, nb, nn = (int(v) for v in sizes[:5])
        L = nf + nb + 3
        levels = np.zeros((L, 3), np.int32)
        counts = np.zeros((L, nn, 2), np.int32)
        fronts = np.zeros((nt, 4), np.int32)
        piv_idx = np.zeros(self.n, np.int32)
        upd_idx = np.zeros(max(nupd, 1), np.int32)
        get(self._h, None, None, _ip(levels), _ip(counts), _ip(fronts), _ip(piv_idx), _ip(upd_idx))
        lv = [dict(rows=int(levels[l, 0]), nwide=int(levels[l, 1]), nnarrow=int(levels[l, 2]), wcount=counts[l, :, 0].copy(),
                   ncount=counts[l, :, 1].copy()) for l in range(L)]
        w, u = fronts[:, 0].copy(), fronts[:, 1].copy()
        piv_lists, upd_lists = _per_front(w, u, piv_idx, upd_idx)
        return {"fused_root": bool(flags[0]), "root_sym": bool(flags[1]), "root_rows": int(flags[2]),
                "root_fine_rows": int(flags[3]), "root_fine_below": int(flags[4]), "stream_once": bool(flags[5]),
                "nnodes": nn, "fwd": lv[:nf], "bwd": lv[nf:nf + nb], "root": lv[-3], "root_fine": lv[-2], "root_rows_level": lv[-1],
                "nfronts": nt, "w": w, "u": u, "parent": fronts[:, 2].copy(), "height": fronts[:, 3].copy(),
                "piv_idx": piv_lists, "upd_idx": upd_lists}

    def fine_root_for(self, nodes):
        return bool(lib().dpgo_debug_spd_solver_fine_root(self._h, int(nodes)))

    def run(self, rhs, out, mask=~0, mask_word=None, class_of=None, scale=1.0, in_place=False):
        a = np.ascontiguousarray(rhs, np.float64)
        o = np.ascontiguousarray(out, np.float64).copy()
        if a.shape != self.shape or o.shape != self.shape:
            raise ValueError("record arrays must be %r" % (self.shape,))
        word = None if mask_word is None else C.byref(C.c_ulonglong(int(mask_word) & (2 ** 64 - 1)))
        cls = None if class_of is None else C.byref(C.c_ulonglong(int(class_of) & (2 ** 64 - 1)))
        rc = lib().dpgo_debug_spd_solver_run(self._h, int(mask) & (2 ** 64 - 1), word, cls, float(scale), int(bool(in_place)),
                                             _dp(a), _dp(o))
        if rc == -2:
            return None
        if rc != 0:
            raise RuntimeError("dpgo_debug_spd_solver_run failed")
        return o

    def refactor(self, values):
        v = np.ascontiguousarray(values, np.float64)
        if v.shape != (self.nval,):
            raise ValueError("one value per stored entry of A")
        rc = lib().dpgo_debug_spd_solver_refactor(self._h, _dp(v))
        if rc != 0:
            raise RuntimeError("not positive definite" if rc == 1 else "dpgo_debug_spd_solver_refactor failed")


def spd_panel_pack_debug(src, rows, pairs=True, mat_off=0, fill=0.0):
    """One solve tile's panel from the host packer of SpdSolverDev::upload (test hook, dpgo_debug_spd_panel_pack; no GPU).
    src: len x count, entry (k, r) of the tile; rows: the tile height of its class (64, 16 or 8).  Returns (panel, info):
    the array of mat_off + panel doubles, filled with `fill` before the packer ran, and a dict ld, pair_kq, mat_off, doubles
    as the tile's descriptor reports them."""
    a = np.ascontiguousarray(src, np.float64)
    if a.ndim != 2:
        raise ValueError("src must be len x count")
    info = np.zeros(4, np.int64)
    args = (int(rows), a.shape[1], a.shape[0], int(bool(pairs)), int(mat_off))
    if lib().dpgo_debug_spd_panel_pack(*args, None, 0, None, 0, info.ctypes.data_as(_LLP)) != 0:
        raise ValueError("dpgo_debug_spd_panel_pack refused the tile")
    panel = np.full(int(mat_off) + int(info[3]), float(fill))
    if lib().dpgo_debug_spd_panel_pack(*args, _dp(a), a.shape[1], _dp(panel), panel.size, info.ctypes.data_as(_LLP)) != 0:
        raise RuntimeError("dpgo_debug_spd_panel_pack failed")
    return panel, {"ld": int(info[0]), "pair_kq": int(info[1]), "mat_off": int(info[2]), "doubles": int(info[3])}


CG_DEBUG_KINDS = ("begin_host", "begin_device", "scal0", "scal1", "scal_begin", "reduce_gate", "reduce")
GATE_OPTIONS = ("max_it", "max_acc", "max_hits0", "max_hits1", "rel_tol", "step_tol", "psi", "phi")   # of a reduce_gate launch
GATE_NODE_SCALARS = ("f", "Fk0", "Fk1", "fobj", "hits0", "hits1")                                     # ... one per local node
GATED_BUFFERS = ("Xk", "Zc", "Zp", "gc", "gp", "Dfc", "Dfp", "GXc", "GXp", "partials", "DfE", "e_w")                             # debug_gated_update
MAX_SLOTS = 32
CG_RECORD_FIELDS = ("sk_M_pk", "sk_M_2", "pk_M_2", "rv", "Delta", "Delta_2", "target", "h_M_norm", "c1", "cr", "al", "kap", "be",
                    "cg_it", "max_it", "live", "stop_ord")


class CgDebugLaunch(C.Structure):
    """dpgo_cg_debug_launch_t"""
    _fields_ = [("kind", C.c_int), ("use_precon", C.c_int), ("max_it", C.c_int), ("slots", C.c_int), ("bits", C.c_ulonglong),
                ("grad_tol", C.c_double), ("pgrad_tol", C.c_double), ("kappa", C.c_double), ("theta", C.c_double),
                ("rv", _DP), ("Delta", _DP), ("target", _DP), ("partials", _DP), ("gate", C.c_void_p)]


class GateDebug(C.Structure):
    """dpgo_gate_debug_t"""
    _fields_ = [(k, C.c_int) for k in ("nslots", "max_it", "max_acc", "max_hits0", "max_hits1")] + \
               [(k, C.c_double) for k in ("rel_tol", "step_tol", "psi", "phi")] + \
               [(k, _DP) for k in ("f", "Fk0", "Fk1", "fobj")] + [("hits0", _IP), ("hits1", _IP)]


class InterUpdateDebug(C.Structure):
    """dpgo_inter_update_debug_t"""
    _fields_ = [(k, C.c_int) for k in ("local", "whole", "quad", "with_Df", "nrecv")] + \
               [(k, _DP) for k in ("Z", "Zprev", "DfE_old", "GX", "X", "Znbr", "recv")] + [("nsrc", _IP)] + \
               [(k, _DP) for k in ("DfE", "g", "w", "sums", "Df", "Z_after", "Znbr_after")]


class CertUpdateDebug(C.Structure):
    """dpgo_cert_update_debug_t"""
    _fields_ = [(k, _DP) for k in ("C", "theta", "V", "W", "P", "SV", "SW", "SP")] + [("ld", C.c_int), ("precondition", C.c_int),
               ("nbr_fill", C.c_double)] + [(k, _DP) for k in ("V_out", "W_out", "P_out", "SV_out", "SW_out", "SP_out", "sums", "nbr")]


class InterIterateDebug(C.Structure):
    """dpgo_inter_iterate_debug_t"""
    _fields_ = [(k, C.c_int) for k in ("local", "whole", "fused", "prox", "gamma_dev")] + \
               [(k, _DP) for k in ("Zc", "Zp", "GXc", "GXp", "Xref", "gamma", "Y", "g", "Df", "Xout", "Xref_after", "sums")]


class NodeGroup:
    """The DPGOHash objects of the nodes hosted by one GPU (one process)."""

    def __init__(self, graph, node_ids, options, device=0):
        self.graph, self.options = graph, options
        self.node_ids = [int(a) for a in node_ids]
        ids = np.asarray(self.node_ids, np.int32)
        h = C.c_void_p()
        if lib().dpgo_group_create(graph._h, _ip(ids), len(ids), C.byref(options), int(device), C.byref(h)) != 0:
            raise RuntimeError("dpgo_group_create failed (no HIP device, or inconsistent input); "
                               "the DPGO hot path has no CPU fallback")
        self._h = h
        self.d = graph.d
        self.sizes = [graph.node_sizes(a) for a in self.node_ids]

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dpgo_group_free(self._h)
            self._h = None

    def __len__(self):
        return len(self.node_ids)

    def __getitem__(self, k):
        return DPGOHash(self, k)

    def _sel(self, locals_):
        if locals_ is None:
            return None, 0
        a = np.asarray(list(locals_), np.int32)
        return _ip(a), len(a)

    def initialize_global(self, X):
        X, ld = _fcol(X)
        return lib().dpgo_group_initialize_global(self._h, _dp(X), ld)

    def update(self, locals_=None):
        p, n = self._sel(locals_)
        return lib().dpgo_group_update(self._h, p, n)

    def iterate(self, locals_=None):
        p, n = self._sel(locals_)
        return lib().dpgo_group_iterate(self._h, p, n)

    def communicate_local(self):
        return lib().dpgo_group_communicate_local(self._h)

    def p2p_self_check(self):
        """Test hook (dpgo_debug_comm_p2p_self): the grouped ncclSend / ncclRecv path of the boundary exchange on a one-rank
        communicator that is its own peer, for the rows this group exports."""
        return lib().dpgo_debug_comm_p2p_self(self._h)

    def step(self, comm=None):
        """iterate() of every node, the boundary exchange of `comm` (a Comm of this group) if any, communicate(), update():
        the body of the driver's loop (dist_pgo.cpp:496-521) in one native call."""
        return lib().dpgo_group_step(self._h, comm._h if comm is not None else None)

    def sync(self):
        return lib().dpgo_group_sync(self._h)

    def stream(self):
        return lib().dpgo_group_stream(self._h)

    # boundary exchange across groups
    def sent_keys(self):
        n = lib().dpgo_group_num_sent(self._h)
        a, b = np.empty(n, np.int32), np.empty(n, np.int32)
        lib().dpgo_group_sent_keys(self._h, _ip(a), _ip(b))
        return a, b

    def set_recv_layout(self, stride, keys_per_rank):
        counts = np.asarray([len(k[0]) for k in keys_per_rank], np.int32)
        nodes = np.ascontiguousarray(np.concatenate([k[0] for k in keys_per_rank]) if len(counts) else [], np.int32)
        poses = np.ascontiguousarray(np.concatenate([k[1] for k in keys_per_rank]) if len(counts) else [], np.int32)
        return lib().dpgo_group_set_recv_layout(self._h, len(counts), int(stride), _ip(counts), _ip(nodes), _ip(poses))

    def set_collectives(self, send_ptr, gathered_ptr, allgather, allreduce):
        """Lend the group an all-gather of its boundary buffer and a sum over the groups (AMM-PGO* with the
        nodes spread over several processes).  allgather() -> 0; allreduce(numpy array) -> 0, in place."""
        def _ag(_user):
            try:
                return int(allgather() or 0)
            except Exception as e:      # an exception must not unwind through the C frames
                sys.stderr.write("allgather callback: %r\n" % (e,))
                return -1

        def _ar(_user, vals, n):
            try:
                a = np.ctypeslib.as_array(vals, shape=(n,))
                return int(allreduce(a) or 0)
            except Exception as e:
                sys.stderr.write("allreduce callback: %r\n" % (e,))
                return -1
        self._cb = (C.CFUNCTYPE(C.c_int, C.c_void_p)(_ag), C.CFUNCTYPE(C.c_int, C.c_void_p, _DP, C.c_int)(_ar))
        return lib().dpgo_group_set_collectives(self._h, C.c_void_p(send_ptr), C.c_void_p(gathered_ptr),
                                                C.cast(self._cb[0], C.c_void_p), C.cast(self._cb[1], C.c_void_p), None)

    def pack_sent(self, dev_ptr):
        return lib().dpgo_group_pack_sent(self._h, C.c_void_p(dev_ptr))

    def unpack_recv(self, dev_ptr):
        return lib().dpgo_group_unpack_recv(self._h, C.c_void_p(dev_ptr))

    def scatter_global(self, X):
        assert X.flags.f_contiguous
        return lib().dpgo_group_scatter_global(self._h, _dp(X), X.shape[0])

    def connect_torch(self):
        """Connect this group to the groups of the other processes of an initialised torch.distributed process group
        (one process per GPU: backend nccl = RCCL; gloo: staged through the host, lets several processes share a GPU
        in tests): the recv lay-out of the boundary poses and the two collectives the library needs when the nodes
        of the graph are spread over several groups (AMM-PGO*, the distributed chordal initialisation, global
        evaluations).  Returns (dist, torch, send, gathered, stream, allgather)."""
        import torch
        import torch.distributed as dist
        world, RS = dist.get_world_size(), (self.d + 1) * self.d
        host = dist.get_backend() == "gloo"          # gloo: staged through pinned host tensors
        keys = self.sent_keys()
        allkeys = [None] * world
        dist.all_gather_object(allkeys, (keys[0].tolist(), keys[1].tolist()))
        stride = max(max(len(k[0]) for k in allkeys), 1)
        self.set_recv_layout(stride, [(np.asarray(k[0], np.int32), np.asarray(k[1], np.int32)) for k in allkeys])
        send = torch.zeros(stride * RS, dtype=torch.float64, device="cuda")
        gathered = torch.zeros(world * stride * RS, dtype=torch.float64, device="cuda")
        send_h = torch.zeros(stride * RS, dtype=torch.float64) if host else None
        gathered_h = torch.zeros(world * stride * RS, dtype=torch.float64) if host else None
        ext = torch.cuda.ExternalStream(self.stream())
        torch.cuda.synchronize()

        def allgather():
            with torch.cuda.stream(ext):
                if host:
                    send_h.copy_(send)
                    dist.all_gather_into_tensor(gathered_h, send_h)
                    gathered.copy_(gathered_h)
                else:
                    dist.all_gather_into_tensor(gathered, send)
            return 0

        def allreduce(vals):
            t = torch.from_numpy(vals.copy())
            if not host:
                t = t.cuda()
            dist.all_reduce(t)                       # same reduction order on every rank: identical branches
            vals[:] = t.cpu().numpy()
            return 0
        if self.set_collectives(send.data_ptr(), gathered.data_ptr(), allgather, allreduce) != 0:
            raise RuntimeError("dpgo_group_set_collectives failed")
        self._torch_link = (dist, torch, send, gathered, ext, allgather)
        return self._torch_link

    def dist_chordal_initialization(self, options=None, X_local=None):
        """The --dist_init true branch of dist_pgo (dist_pgo.cpp:144-416): returns (X, objectives) -- the initial
        guess ((d+1)N x d) and the stage objectives sampled every 20 iterations."""
        o = options or DChordalOptions()
        N, d = self.graph.num_poses, self.d
        X = np.zeros(((d + 1) * N, d), order="F")
        cap = sum((o.iters[k] + 19) // 20 for k in range(4))
        obj, cnt = np.zeros(max(cap, 1)), C.c_int(cap)
        xl, ldl = (None, 0)
        if X_local is not None:
            Xl, ldl = _fcol(X_local)
            xl = _dp(Xl)
        if lib().dpgo_group_dist_chordal_initialization(self._h, C.byref(o), xl, ldl, _dp(X), X.shape[0], _dp(obj),
                                                        C.byref(cnt)) != 0:
            raise RuntimeError("distributed chordal initialisation failed")
        return X, obj[:cnt.value]

    def evaluate(self, X, want_grad=False):
        """DPGOStar::evaluate_f / evaluate_grad at an arbitrary global X: (F, |grad F|^2[, grad]) summed over
        this group's nodes (over all groups when collectives are attached)."""
        X, ld = _fcol(X)
        F, g2 = C.c_double(), C.c_double()
        G = np.zeros_like(X, order="F") if want_grad else None
        if lib().dpgo_group_evaluate(self._h, _dp(X), ld, C.byref(F), C.byref(g2), _dp(G) if want_grad else None,
                                     ld if want_grad else 0) != 0:
            raise RuntimeError("dpgo_group_evaluate failed")
        return (F.value, g2.value, G) if want_grad else (F.value, g2.value)

    def certify(self, X, eta=1e-3, tau=1e-6, max_iters=2000, precondition=True, stop_on_negative=True, seed=0, V0=None,
                refresh_every=50):
        """Is X the global minimum of the trivial-loss problem?  LOBPCG with block size d on the certificate matrix
        S = M - Lambda(X) (SESyncProblem::verify_solution, C++/SESync/src/SESyncProblem.cpp:375-468; fast_verification
        STEP 2, C++/SESync/src/SESync_utils.cpp:765-826).  Returns (CertResult, x): x is a unit vector of length (d+1)N,
        theta = x' S x and residual = |S x - theta x| come from one fresh product with it, and status is
        CERT_NEGATIVE (theta < -eta/2: x proves lambda_min(S) < -eta/2), CERT_NONNEGATIVE (column 0 converged with
        theta >= -eta/2 -- evidence, NOT proof: a converged Ritz pair need not be the smallest one; the proof, a
        Cholesky factorisation of S + eta I, is cert_factor / verify) or CERT_UNDECIDED (max_iters
        reached).  stationarity = |S X|_F is the Riemannian gradient norm: the certificate only means something at a
        critical point.  The group must have the trivial loss and host every node; the optimiser's state is untouched.
        V0: the initial block ((d+1)N x d), default seeded Gaussians."""
        X, ld = _fcol(X)
        o, V0, v0, ldv0 = _cert_args(X, "certify", eta, tau, max_iters, precondition, stop_on_negative, refresh_every, seed, V0)
        res = CertResult()
        x = np.zeros(X.shape[0])
        if lib().dpgo_group_certify(self._h, _dp(X), ld, C.byref(o), v0, ldv0, C.byref(res), _dp(x), x.shape[0]) != 0:
            raise RuntimeError("dpgo_group_certify failed (robust loss, a group that does not host every node, or bad sizes)")
        return res, x

    def cert_factor(self, X, eta=1e-3, max_factor_bytes=0):
        """The proof: fast_verification STEP 1 (C++/SESync/src/SESync_utils.cpp:731-754), the Cholesky factorisation of
        S(X) + eta I on the device.  Returns a CertFactor: outcome CERT_FACTOR_PD (lambda_min(S) > -eta, up to the
        rounding of the factorisation), CERT_FACTOR_NOT_PD (a non-positive pivot: lambda_min(S) <= -eta) or
        CERT_FACTOR_SKIPPED (the analysis predicts more device memory than max_factor_bytes, when > 0, or than half of
        what is free: nothing was allocated), with the elimination tree's sizes, the pivot range, stationarity =
        |S X|_F and the host seconds of the analysis and of the numeric phase."""
        X, ld = _fcol(X)
        f = CertFactor()
        if lib().dpgo_group_cert_factor(self._h, _dp(X), ld, float(eta), int(max_factor_bytes), C.byref(f)) != 0:
            raise RuntimeError("dpgo_group_cert_factor failed (robust loss, a group that does not host every node, or bad sizes)")
        return f

    def verify(self, X, eta=1e-3, tau=1e-6, max_iters=2000, precondition=True, stop_on_negative=True, seed=0, V0=None,
               refresh_every=50, max_factor_bytes=0):
        """fast_verification (SESync_utils.cpp:721-830): cert_factor first, certify's search only when the factorisation
        did not succeed.  Returns (CertResult, x, CertFactor).  CERT_FACTOR_PD: status CERT_PROVEN, iterations 0, x zero;
        CERT_FACTOR_NOT_PD: certify's result, except that NONNEGATIVE -- which the factorisation has just refuted --
        becomes UNDECIDED (theta and residual kept); CERT_FACTOR_SKIPPED: certify's result unchanged.  PROVEN is a
        floating-point statement about S(X) and means "global minimum" only where stationarity is small (the header
        include/dpgo_amd.h has the warning example)."""
        X, ld = _fcol(X)
        o, V0, v0, ldv0 = _cert_args(X, "verify", eta, tau, max_iters, precondition, stop_on_negative, refresh_every, seed, V0)
        res, f = CertResult(), CertFactor()
        x = np.zeros(X.shape[0])
        if lib().dpgo_group_verify(self._h, _dp(X), ld, C.byref(o), int(max_factor_bytes), v0, ldv0, C.byref(res), _dp(x),
                                   x.shape[0], C.byref(f)) != 0:
            raise RuntimeError("dpgo_group_verify failed (robust loss, a group that does not host every node, or bad sizes)")
        return res, x, f

    def cert_matrix(self, X, eta):
        """Debug: the matrix cert_factor factors, S(X) + eta I, read back from the device: CSR (ptr, col, val) on the
        unknowns (d+1) g + r of the global poses g (r = 0 the translation, r = 1..d the rows of Y_g), every stored
        (d+1) x (d+1) block dense."""
        X, ld = _fcol(X)
        return _csr_out((self.d + 1) * self.graph.num_poses, "dpgo_group_cert_matrix",
                        lambda *csr: lib().dpgo_group_cert_matrix(self._h, _dp(X), ld, float(eta), *csr))

    def covariance(self, X, anchor=0, pairs=None, max_bytes=0):
        """Marginal pose covariances at X (dpgo_group_covariance): the inverse of the Riemannian Hessian in tangent
        coordinates -- dof = d + d (d - 1) / 2 per pose: the translation increment in the world frame, then omega with
        R <- R Exp(hat(omega)) in the body frame -- with the global pose `anchor` held fixed.  Trivial-loss groups that host
        every node, like the certificate.  pairs: (npairs, 2) global poses, each an edge of the graph (anything else
        raises).  Returns (marginals (N, dof, dof), cross (npairs, dof, dof), CovResult); the blocks that involve the anchor
        are zero.  outcome COV_OK, COV_NOT_PD (the anchored Hessian is not positive definite; zero blocks) or COV_SKIPPED
        (the analysis predicts more device bytes than max_bytes, when > 0, or than half of what is free: nothing of the
        factor was allocated, the predicted sizes are filled in)."""
        X, ld = _fcol(X)
        marg, cross, pair_args = _pairs_arg(pairs, self.graph.num_poses, _dof(self.d))
        r = CovResult()
        if lib().dpgo_group_covariance(self._h, _dp(X), ld, int(anchor), int(max_bytes), *pair_args, C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_covariance failed (robust loss, a group that does not host every node, an anchor or "
                               "pair outside the graph, a pair that is not an edge, or bad sizes)")
        return marg, cross, r

    def pair_covariance(self, X, pairs, anchor=0, candidates=None, max_bytes=0, threshold=None):
        """Joint covariances of arbitrary pose pairs at X and the loop-closure gate (dpgo_group_pair_covariance): the columns
        of the inverse of `covariance`'s anchored Hessian that belong to the poses of `pairs` ((npairs, 2) global poses, any
        two: no edge needed, p == q and the anchor allowed), solved for on the device.  candidates: None, or one candidate
        measurement per pair as a tuple (R (npairs, d, d), t (npairs, d), kappa (npairs), tau (npairs)).
        Returns a dict: joint (npairs, 3, dof, dof): Sigma_pp, Sigma_pq (rows of p, columns of q, as covariance's cross),
        Sigma_qq; rel (npairs, dof, dof): the covariance of T_p^-1 T_q in covariance's perturbation; result (PairsResult); and
        with candidates d2 (npairs), not_pd (npairs, bool), residual (npairs, dof) -- d2 = r' (rel + Omega^-1)^-1 r with
        Omega = blkdiag(tau I, 2 kappa I); with `threshold` (the chi-square quantile of your choice, dof degrees of freedom)
        also accept = d2 <= threshold where the innovation covariance is positive definite.  outcome PAIRS_OK, PAIRS_NOT_PD
        (zero outputs) or PAIRS_SKIPPED (more device bytes than max_bytes, when > 0, or than half of what is free).  No block
        of a selected inversion is stored: this may run where covariance is SKIPPED."""
        X, ld = _fcol(X)
        gated, joint, rel, gate, pair_args = _pair_cov_arg(self.d, pairs, candidates)
        r = PairsResult()
        if lib().dpgo_group_pair_covariance(self._h, _dp(X), ld, int(anchor), int(max_bytes), *pair_args, C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_pair_covariance failed (robust loss, a group that does not host every node, an anchor "
                               "or pose outside the graph, a candidate weight that is not positive, or bad sizes)")
        return pairs_output(joint, rel, gate, r, gated, threshold)

    def joint_marginal(self, X, keep, anchor=0, base=None, want_info=True, max_bytes=0):
        """The joint marginal of a SET of poses at X (dpgo_group_joint_marginal): `keep` lists distinct global poses in any
        order, and the outputs follow that order.  base None: the absolute form, cov = (H^-1)_KK of `covariance`'s anchored
        Hessian, n = dof K (the anchor may not be kept: raises).  base a member of keep (K >= 2): the relative form, the joint
        covariance of T_base^-1 T_k of the other kept poses in list order, n = dof (K - 1), in pair_covariance's perturbation
        of a relative pose; the anchor may then be kept, or be the base.  X should be a critical point (polish).
        Returns a dict: cov (n, n), symmetric bit for bit; info (n, n) = cov^-1 and logdet = log det cov with want_info (else
        None) -- in the absolute form info is the Schur complement of the anchored Hessian onto keep; order: the poses of the
        dof-blocks of cov; result (MargResult).  outcome MARG_OK, MARG_NOT_PD (zero outputs) or MARG_SKIPPED (more device bytes
        than max_bytes, when > 0, or than half of what is free); result.info_not_pd: cov is delivered, info and logdet are
        zeros."""
        X, ld = _fcol(X)
        cov, info, logdet, order, args = _marg_arg(self.d, keep, base, want_info)
        r = MargResult()
        if lib().dpgo_group_joint_marginal(self._h, _dp(X), ld, args[0], args[1], int(anchor), args[2], int(bool(want_info)),
                                           int(max_bytes), _dp(cov), _dp(info), _dp(logdet), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_joint_marginal failed (robust loss, a group that does not host every node, an anchor or "
                               "pose outside the graph, a pose kept twice, the anchor kept without a base, or a base that is "
                               "not one of at least two kept poses)")
        return marg_output(cov, info, logdet, order, r, want_info)

    def candidate_set(self, X, pairs, candidates, anchor=0, budget=0, d2_max=0.0, want_joint=True, want_cov=True, max_bytes=0):
        """Joint compatibility and budgeted selection of loop-closure candidates at X (dpgo_group_candidate_set).  pairs (m, 2):
        global poses, p != q; a pair may repeat, pairs may share poses, either end may be the anchor.  candidates: the tuple
        (R, t, kappa, tau) of pair_covariance, or (m, d^2 + d + 2) in pack_candidates' layout.  X should be a critical point
        (polish).  With n = dof m, returns a dict:
          cov, S         (n, n) with want_cov (else None): J Sigma_KK J^T -- its diagonal blocks are pair_covariance's rel -- and
                         cov + blkdiag(Omega_i^-1); symmetric bit for bit
          residual       (n,): pair_covariance's residuals, stacked
          info, logdet, d2_joint, gain_all   with want_joint (else None; zeros under result.joint_not_pd): S^-1, log det S,
                         r^T S^-1 r -- the candidates' compatibility with the graph TOGETHER -- and the information they would
                         add together, 1/2 (log det S - sum log det Omega_i^-1)
          selected       (n_selected,): with budget > 0 the greedy choice by conditional information gain, in order; a candidate
                         is eligible iff its conditional covariance is positive definite and (d2_max <= 0 or its CONDITIONAL
                         d2 <= d2_max); ties go to the lowest index
          steps          (n_selected, 4): index, gain, d2, the number of eligible candidates at that step
          gain_selected, d2_selected   the sums over the steps: 1/2 (log det S_sel - log det R_sel) and r_sel^T S_sel^-1 r_sel
          poses          the distinct end poses in order of first appearance
          result         CandResult; outcome CAND_OK, CAND_NOT_PD (zero outputs) or CAND_SKIPPED (more device bytes than
                         max_bytes, when > 0, or than half of what is free)."""
        X, ld = _fcol(X)
        a, head, tail = _cand_arg(self.d, pairs, candidates, budget, want_joint, want_cov)
        r = CandResult()
        if lib().dpgo_group_candidate_set(self._h, _dp(X), ld, *head, int(anchor), a["budget"], float(d2_max), int(bool(want_joint)),
                                          int(max_bytes), *tail, C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_candidate_set failed (robust loss, a group that does not host every node, an anchor or "
                               "pose outside the graph, a candidate that joins a pose to itself, or a weight that is not positive)")
        return cand_output(a, r, want_joint)

    def sensitivity(self, X, upstream, anchor=0, max_bytes=0, graph=None, want_adjoint=False):
        """Measurement sensitivities at X by implicit differentiation on the device (dpgo_group_sensitivity): for k scalars
        L_l(X*) whose tangent gradients at X are the columns of `upstream` ((dof N, k), or (dof N,) for one; by global pose, in
        `covariance`'s coordinates: see tangent_gradient and unit_upstream), the adjoints lambda_l = H^-1 c_l on `covariance`'s
        anchored Hessian and, for every edge of `graph` (default: the group's own, which fixes the edge order),
        dL_l / d(kappa, tau, t~[0..d), eta[0..dof - d)) with t~ + dt~ and R~ <- R~ Exp(hat(eta)).  X should be a critical point
        (`polish`): result.stationarity says whether it is.  Returns (SensResult, sens) with sens (k, num_edges, 2 + dof), and
        with want_adjoint also lambda (dof N, k), zeros on the anchor.  outcome SENS_OK, SENS_NOT_PD (zero outputs) or
        SENS_SKIPPED (more device bytes than max_bytes, when > 0, or than half of what is free; zero outputs).  A column's
        bits do not depend on the other columns of the call.  Trivial-loss groups that host every node."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        n = _dof(self.d) * self.graph.num_poses
        U_ = np.asarray(upstream, np.float64)
        U_ = np.asfortranarray(U_.reshape(-1, 1) if U_.ndim == 1 else U_)
        if U_.ndim != 2 or U_.shape[0] != n or U_.shape[1] < 1:
            raise ValueError("sensitivity: upstream must be (dof N, k) with k >= 1")
        k = U_.shape[1]
        sens = np.zeros((k, g_.num_edges, 2 + _dof(self.d)))
        adj = np.zeros((n, k), order="F") if want_adjoint else None
        r = SensResult()
        if lib().dpgo_group_sensitivity(self._h, g_._h, _dp(X), ld, int(anchor), int(max_bytes), _dp(U_), n, k, _dpn(adj), _dp(sens),
                                        C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_sensitivity failed (robust loss, a group that does not host every node, a graph that is "
                               "not the group's, an anchor outside the graph, an upstream entry that is not finite, or bad sizes)")
        return (r, sens, adj) if want_adjoint else (r, sens)

    def edge_reliability(self, X, edges=None, anchor=0, method=0, max_bytes=0, graph=None):
        """Per-edge reliability at X (dpgo_group_edge_reliability): for every edge of `graph` (default: the group's own, which
        numbers the edges), or for the listed indices -- any order, repeats allowed -- the leave-one-out chi-square d2_loo =
        r' C^-1 r on the residual covariance C = Omega^-1 - Sigma_rel, the residual r_loo the edge would have at the solution
        of the graph without it, the influence of removing it, the redundancy numbers and d2_own = r' Omega r, from the blocks
        the selected inversion leaves on the device (method RELY_SELINV), from `pair_covariance`'s block solves (RELY_SOLVE),
        or from whichever is not refused (RELY_AUTO, the default).  X should be a critical point (`polish`).  Returns a dict:
        records (n, 6 + 2 dof) as the C ABI lays them out; its columns d2_loo, flag (int: 0, 1 = C not positive definite and
        d2_loo, influence, r_loo zero, 2 = an edge without weight, all zero), redundancy, redundancy_trans, d2_own, influence,
        residual (n, dof), r_loo (n, dof); rel (n, dof, dof); joint (n, 3, dof, dof) as `pair_covariance`; result (RelyResult).
        outcome RELY_OK, RELY_NOT_PD (zero outputs) or RELY_SKIPPED (zero outputs, both byte predictions filled).  No threshold
        is applied.  Trivial-loss groups that host every node."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        records, rel, joint, edge_args = _rely_arg(g_, edges)
        r = RelyResult()
        if lib().dpgo_group_edge_reliability(self._h, g_._h, _dp(X), ld, int(anchor), int(max_bytes), int(method), *edge_args,
                                             _dp(records), _dp(rel), _dp(joint), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_edge_reliability failed (robust loss, a group that does not host every node, a graph that "
                               "is not the group's, an anchor or an edge index outside the graph, an unknown method, or bad sizes)")
        return rely_output(g_.d, records, rel, joint, r)

    def polish(self, X, anchor=0, max_bytes=0, **opts):
        """Newton polish (dpgo_group_polish): damped Riemannian Newton steps from X -- Levenberg-Marquardt on the anchored
        tangent-space Hessian of `covariance`, factored and solved on the device -- until the tangent gradient is at rounding
        level (|g| <= rel_tol hmax, or grad_tol when > 0) or max_steps are spent.  Trivial-loss groups that host every node;
        the global pose `anchor` is held fixed.  opts: the fields of PolishOptions (max_steps 20, max_tries 8, rel_tol 1e-9,
        grad_tol 0).  Returns (Xout, PolishResult, log): the new point (X itself for POLISH_SKIPPED), the result struct, and
        one row per iteration of (F0, |g|, mu at entry, rho of the accepted try, tries).  The optimiser's state is not
        touched."""
        X, ld, o, Xout, log = _polish_arg(X, anchor, opts)
        r = PolishResult()
        if lib().dpgo_group_polish(self._h, _dp(X), ld, C.byref(o), int(max_bytes), _dp(Xout), Xout.shape[0], _dp(log), len(log),
                                   C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_polish failed (robust loss, a group that does not host every node, an anchor outside "
                               "the graph, or bad sizes or options)")
        return Xout, r, _polish_log(log, r)

    def hessian_modes(self, X, k, anchor=0, max_bytes=0, **opts):
        """The k smallest eigenpairs of `covariance`'s anchored Hessian H at X (dpgo_group_hessian_modes): shift-invert block
        subspace iteration with Rayleigh-Ritz on the covariance's factor.  An indefinite H is an input -- the factor is that of
        H + mu I, the values are those of H -- and at a polished minimum 1 / values[0] is the largest eigenvalue of the
        covariance.  1 <= k <= 60, k <= dof (N - 1).  opts: the fields of ModesOptions (guard 4, max_iters 100, max_tries 8,
        want_escape 0, rel_tol 1e-8, shift 0, seed 1).  Returns a dict:
          values     (k,): lambda_j ascending;  residuals (k,): |H v_j - lambda_j v_j| from the iteration's recurrence
          vectors    (k, dof N): row j the unit vector v_j, pose-major by global pose, zeros on the anchor
          energy     (k, N): |v_j|^2 per pose; rows sum to 1
          X_escape   with want_escape: where lambda_0 < 0 a lower point along v_0 (result.escaped, F_escape, escape_alpha),
                     otherwise X; None without
          result     ModesResult; outcome MODES_CONVERGED, MODES_MAX_ITERS (the last iteration's pairs), MODES_STALLED or
                     MODES_SKIPPED (more device bytes than max_bytes, when > 0, or than half of what is free).
        The optimiser's state is not touched."""
        X, ld = _fcol(X)
        k = int(k)
        o = ModesOptions(**opts)
        N, dof = self.graph.num_poses, _dof(self.d)
        kk = max(k, 1)
        values, residuals, vectors, energy = np.zeros(kk), np.zeros(kk), np.zeros((kk, dof * N)), np.zeros((kk, N))
        Xe = np.array(X, order="F") if o.want_escape else None
        r = ModesResult()
        if lib().dpgo_group_hessian_modes(self._h, _dp(X), ld, int(anchor), k, C.byref(o), int(max_bytes), _dp(values), _dp(residuals),
                                          _dp(vectors), _dp(energy), _dpn(Xe), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_hessian_modes failed (robust loss, a group that does not host every node, an anchor outside "
                               "the graph, k outside 1 ... min(60, dof (N - 1)), or bad sizes or options)")
        return {"values": values, "residuals": residuals, "vectors": vectors, "energy": energy, "X_escape": Xe, "result": r}

    def robust_polish(self, X, loss, loss_reg=0.25, curvature=1, anchor=0, max_bytes=0, graph=None, **opts):
        """Newton polish of the ROBUST objective F = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e) (dpgo_group_robust_polish):
        `polish`'s loop with the robust F, gradient and Hessian written on the device.  curvature 1: the true Hessian, with the
        curvature 2 rho'' of the loss (quadratic convergence); 0: the re-weighted one (an IRLS-Newton step, linear).  The group is
        a trivial-loss group that hosts every node; graph (default: the group's own) gives the edges and the inter rule.
        Returns (Xout, PolishResult, log, EdgeSummary of the final point): as `polish`, the F fields the robust F."""
        X, ld, o, Xout, log = _polish_arg(X, anchor, opts)
        r, sm = PolishResult(), EdgeSummary()
        if lib().dpgo_group_robust_polish(self._h, (graph or self.graph)._h, _dp(X), ld, int(loss), float(loss_reg), int(curvature),
                                          C.byref(o), int(max_bytes), _dp(Xout), Xout.shape[0], _dp(log), len(log), C.byref(r),
                                          C.byref(sm)) != 0:
            raise RuntimeError("dpgo_group_robust_polish failed (a robust-loss group, a group that does not host every node, a graph "
                               "that is not the group's, a bad loss, loss_reg, curvature or anchor, or bad sizes or options)")
        return Xout, r, _polish_log(log, r), sm

    def gnc(self, graph, X, opt=None, robust_set=None, max_bytes=0):
        """Graduated non-convexity (dpgo_group_gnc): GNC-TLS or GNC-GM outlier rejection on the device.  Level 0 solves with
        unit weights; every later level re-weights the robust set -- the inter-node edges of `graph`, or the edges with
        robust_set[e] != 0 -- in closed form from the surrogate rho_mu and solves the weighted problem with `polish`'s loop,
        while mu walks the surrogate from convex to the truncated (TLS) or Geman-McClure loss.  The group is a trivial-loss
        group that hosts every node.  opt: GncOptions (None: the defaults).  Returns (Xout, weights, GncResult, log): the
        point (X itself for GNC_SKIPPED), one weight per edge, the result struct, and one row per level k >= 1 of (mu,
        F_mu(X_{k-1}), F_w(X_{k-1}), F_w(X_k), F_mu(X_k), inner steps, inner outcome, the counts of w == 0, w == 1 and
        0 < w < 1 over the robust set)."""
        return self._gnc_call("gnc", GncResult(), graph, X, opt, robust_set, max_bytes, "a bad kind, barc2, mu_step, max_levels or anchor")

    def _gnc_call(self, name, r, graph, X, opt, robust_set, max_bytes, bad):
        # what `gnc` and `ml_gnc` share: the outputs, the robust set's check, the call and its error (bad: what it may refuse)
        X, ld = _fcol(X)
        o = GncOptions() if opt is None else opt
        Xout, w = np.array(X, order="F"), np.ones(graph.num_edges)
        log = np.zeros((max(int(o.max_levels), 0), 10))
        rs = None if robust_set is None else np.ascontiguousarray(robust_set, np.int32)
        if rs is not None and rs.shape != (graph.num_edges,):
            raise ValueError("%s: robust_set must have one entry per edge" % name)
        fn = getattr(lib(), "dpgo_group_" + name)
        if fn(self._h, graph._h, _dp(X), ld, C.byref(o), None if rs is None else _ip(rs), int(max_bytes), _dp(Xout), Xout.shape[0],
              _dp(w), _dp(log) if len(log) else None, len(log), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_%s failed (a robust-loss group, a group that does not host every node, a graph that is "
                               "not the group's, %s, or bad sizes or options)" % (name, bad))
        return Xout, w, r, log[:r.levels].copy()

    def gnc_eval(self, graph, X, kind, mu, barc2, robust_set=None, w_in=None, w_start=None):
        """Debug: one edge pass of graduated non-convexity at X (dpgo_group_gnc_eval).  w_in None: WEIGH -- the weight array
        starts as w_start (default: ones) and weight_mu(s_e) is written on the robust set; otherwise FIXED on w_in.  Returns
        (s_rot, s_trans, w, sums): w the array behind the pass; sums = (sum_{not R} s, sum_R w s, sum_R rho_mu(s), max_R s,
        min_R w, the counts of w == 0, w == 1, 0 < w < 1 over R)."""
        m = graph.num_edges
        head, w = self._gnc_eval_args("gnc_eval", graph, X, kind, mu, barc2, robust_set, w_in, w_start)
        sr, st, sums = np.zeros(m), np.zeros(m), np.zeros(8)
        if lib().dpgo_group_gnc_eval(*head, _dp(sr), _dp(st), _dp(w), _dp(sums)) != 0:
            raise RuntimeError("dpgo_group_gnc_eval failed (a robust-loss group, a group that does not host every node, a graph that "
                               "is not the group's, a bad kind, mu or barc2, or bad sizes)")
        return sr, st, w, sums

    def _gnc_eval_args(self, name, graph, X, kind, mu, barc2, robust_set, w_in, w_start):
        # what `gnc_eval` and `ml_gnc_eval` share: the call's arguments up to and including w_in, and the weight array behind the
        # pass (a pointer of ndarray.ctypes.data_as holds a reference to its array, so the copies made here outlive the call)
        X, ld = _fcol(X)
        m = graph.num_edges
        rs = None if robust_set is None else np.ascontiguousarray(robust_set, np.int32)
        wi = None if w_in is None else np.ascontiguousarray(w_in, np.float64)
        w = np.ones(m) if w_start is None else np.array(w_start, np.float64)
        if any(a is not None and a.shape != (m,) for a in (rs, wi, w)):
            raise ValueError("%s: robust_set, w_in and w_start must have one entry per edge" % name)
        return (self._h, graph._h, _dp(X), ld, int(kind), float(mu), float(barc2), None if rs is None else _ip(rs), _dpn(wi)), w

    def robust_covariance(self, X, loss, loss_reg=0.25, curvature=1, anchor=0, pairs=None, max_bytes=0, graph=None):
        """Marginal pose covariances of the ROBUST objective at X (dpgo_group_robust_covariance): `covariance` on the true
        Hessian (curvature 1) or the re-weighted one (curvature 0).  COV_NOT_PD is a legitimate answer where the negative
        curvature of the loss wins.  Returns (marginals, cross, CovResult) as `covariance`; stationarity = |S_w X|_F."""
        X, ld = _fcol(X)
        marg, cross, pair_args = _pairs_arg(pairs, self.graph.num_poses, _dof(self.d))
        r = CovResult()
        if lib().dpgo_group_robust_covariance(self._h, (graph or self.graph)._h, _dp(X), ld, int(loss), float(loss_reg), int(curvature),
                                              int(anchor), int(max_bytes), *pair_args, C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_robust_covariance failed (a robust-loss group, a group that does not host every node, a "
                               "graph that is not the group's, a bad loss, loss_reg, curvature, anchor or pair, or bad sizes)")
        return marg, cross, r

    def robust_sensitivity(self, X, upstream, loss, loss_reg=0.25, anchor=0, max_bytes=0, graph=None, want_adjoint=False):
        """Measurement sensitivities at a critical point X of the ROBUST objective (dpgo_group_robust_sensitivity), the loss
        threshold delta = loss_reg one more parameter: `sensitivity` with the adjoints lambda_l = H^-1 c_l on the TRUE robust
        Hessian of `robust_covariance` (curvature 1) and, per edge, dL_l/dtheta_e = -[w_e d phi_e/d theta_e + (c_e / 2) phi_e
        d s_e/d theta_e].  X should come from `robust_polish` with the same loss and loss_reg: result.stationarity = |S_w X|_F.
        Returns (SensResult, sens, dloss_reg) with sens (k, num_edges, 3 + dof) -- dL_l/d(kappa, tau, t~, eta) and, last, the
        edge's term of dL_l/d delta -- and dloss_reg (k,) = dL_l/d delta, those terms summed in edge order; with want_adjoint
        also lambda (dof N, k).  Intra edges carry `sensitivity`'s values, an edge whose weight is exactly 0 exact zeros;
        LOSS_NONE gives `sensitivity`'s values and zero delta terms.  SENS_NOT_PD (zero outputs) is a legitimate answer under
        Geman-McClure and Welsch; SENS_SKIPPED as in `sensitivity`.  A column's bits do not depend on the other columns."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        n = _dof(self.d) * self.graph.num_poses
        U_ = np.asarray(upstream, np.float64)
        U_ = np.asfortranarray(U_.reshape(-1, 1) if U_.ndim == 1 else U_)
        if U_.ndim != 2 or U_.shape[0] != n or U_.shape[1] < 1:
            raise ValueError("robust_sensitivity: upstream must be (dof N, k) with k >= 1")
        k = U_.shape[1]
        sens, dreg = np.zeros((k, g_.num_edges, 3 + _dof(self.d))), np.zeros(k)
        adj = np.zeros((n, k), order="F") if want_adjoint else None
        r = SensResult()
        if lib().dpgo_group_robust_sensitivity(self._h, g_._h, _dp(X), ld, int(loss), float(loss_reg), int(anchor), int(max_bytes),
                                               _dp(U_), n, k, _dpn(adj), _dp(sens), _dp(dreg), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_robust_sensitivity failed (a robust-loss group, a group that does not host every node, a "
                               "graph that is not the group's, a bad loss, loss_reg or anchor, an upstream entry that is not "
                               "finite, or bad sizes)")
        return (r, sens, dreg, adj) if want_adjoint else (r, sens, dreg)

    def robust_hessian(self, X, loss, loss_reg=0.25, curvature=1, anchor=0, graph=None, edges=False):
        """Debug: the anchored Hessian of the robust objective as the device wrote it (dpgo_group_robust_hessian).  Returns
        (ptr, col, val, g, F, w, c): the CSR of `cov_hessian`, the tangent gradient (dof N by global pose, zeros on the
        anchor), the robust F, and per edge the weight w and the curvature c = 2 rho''.  edges=True: (s_rot, s_trans, rho) of
        every edge are appended as an eighth item -- what EdgeEval.run returns, bit for bit."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        n = _dof(self.d) * self.graph.num_poses
        args = (self._h, g_._h, _dp(X), ld, int(loss), float(loss_reg), int(curvature), int(anchor))
        g, F, w, c = np.zeros(n), C.c_double(0), np.zeros(g_.num_edges), np.zeros(g_.num_edges)
        per = [np.zeros(g_.num_edges) for _ in range(3)]
        ptr, col, val = _csr_out(n, "dpgo_group_robust_hessian",
                                 lambda *csr: lib().dpgo_group_robust_hessian(*args, *csr, *[None] * 7),
                                 lambda *csr: lib().dpgo_group_robust_hessian(*args, *csr, _dp(g), C.byref(F), _dp(w), _dp(c),
                                                                              *[_dp(a) for a in per]))
        return (ptr, col, val, g, F.value, w, c) + ((tuple(per),) if edges else ())

    def ml_polish(self, X, anchor=0, max_bytes=0, graph=None, **opts):
        """Maximum-likelihood refinement on the full information matrices (dpgo_group_ml_polish): `polish`'s loop on
        F_ml = 1/2 sum_e r_e' Omega_e r_e with r_e = (R~^T (R_i^T (t_j - t_i) - t~), Log(R~^T R_i^T R_j)) and the Gauss-Newton
        Hessian sum J' Omega J -- what g2o, GTSAM and Ceres minimise on the same file.  Start it from the isotropic polished
        point.  The group is a trivial-loss group that hosts every node; graph (default: the group's own) gives the edges and
        their Omega (Graph.edge_information).  Returns (Xout, MlResult, log): as `polish`, the F fields F_ml."""
        X, ld, o, Xout, log = _polish_arg(X, anchor, opts)
        r = MlResult()
        if lib().dpgo_group_ml_polish(self._h, (graph or self.graph)._h, _dp(X), ld, C.byref(o), int(max_bytes), _dp(Xout),
                                      Xout.shape[0], _dp(log), len(log), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_ml_polish failed (a robust-loss group, a group that does not host every node, a graph "
                               "that is not the group's, an anchor outside it, an information matrix that is not symmetric "
                               "positive definite, or bad sizes or options)")
        return Xout, r, _polish_log(log, r.polish)

    def ml_covariance(self, X, anchor=0, pairs=None, max_bytes=0, graph=None):
        """Marginal pose covariances of the maximum-likelihood objective at X (dpgo_group_ml_covariance): `covariance` on
        H = sum J' Omega J, the Fisher information -- the marginals g2o and GTSAM hand out.  Returns and outcomes as
        `covariance`; result.stationarity is the norm of the tangent gradient of F_ml."""
        X, ld = _fcol(X)
        marg, cross, pair_args = _pairs_arg(pairs, self.graph.num_poses, _dof(self.d))
        r = CovResult()
        if lib().dpgo_group_ml_covariance(self._h, (graph or self.graph)._h, _dp(X), ld, int(anchor), int(max_bytes), *pair_args,
                                          C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_ml_covariance failed (a robust-loss group, a group that does not host every node, a "
                               "graph that is not the group's, an anchor or pair outside it, a pair that is not an edge, or an "
                               "information matrix that is not symmetric positive definite)")
        return marg, cross, r

    def ml_edge_reliability(self, X, edges=None, anchor=0, method=0, max_bytes=0, graph=None):
        """`edge_reliability` on the full information matrices (dpgo_group_ml_edge_reliability): the Hessian is
        H = sum J' Omega J with the graph's Omega, rel = J Sigma_joint J' with the exact Jacobians of the ML residual, and
        d2_loo = r' (Omega^-1 - rel)^-1 r, r_loo, influence, the redundancies and d2_own = chi2_e are measured in Omega -- a
        chi-square quantity of dof degrees of freedom for anisotropic noise.  X should be an `ml_polish` point.  Returns
        `edge_reliability`'s dict (flag 2 does not occur); result.stationarity is the norm of the tangent gradient of F_ml, and
        the redundancies sum to dof (m - N + 1)."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        records, rel, joint, edge_args = _rely_arg(g_, edges)
        r = RelyResult()
        if lib().dpgo_group_ml_edge_reliability(self._h, g_._h, _dp(X), ld, int(anchor), int(max_bytes), int(method), *edge_args,
                                                _dp(records), _dp(rel), _dp(joint), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_ml_edge_reliability failed (a robust-loss group, a group that does not host every node, a "
                               "graph that is not the group's, an anchor or an edge index outside it, an unknown method, or an "
                               "information matrix that is not symmetric positive definite)")
        return rely_output(g_.d, records, rel, joint, r)

    def ml_pair_gate(self, X, pairs, candidates, anchor=0, max_bytes=0, threshold=None, graph=None):
        """The loop-closure gate of `pair_covariance` on the full information matrices (dpgo_group_ml_pair_gate): for every
        pair (p, q) -- p == q and the anchor allowed -- with candidates = (R (n, d, d), t (n, d), info (n, dof, dof), each
        symmetric positive definite), d2 = r' (rel + info^-1)^-1 r with the ML residual r and rel = J Sigma_joint J' on
        H = sum J' Omega J.  Returns `pair_covariance`'s dict (joint, rel, result, d2, not_pd, residual; accept with a
        threshold)."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        d, dof = g_.d, _dof(g_.d)
        P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
        n = len(P)
        R, t, info = candidates
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(n, d * d))
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(n, d))
        info = np.ascontiguousarray(np.asarray(info, np.float64).reshape(n, dof * dof))
        joint, rel, gate = np.zeros((n, 3, dof, dof)), np.zeros((n, dof, dof)), np.zeros((n, 2 + dof))
        r = PairsResult()
        if lib().dpgo_group_ml_pair_gate(self._h, g_._h, _dp(X), ld, int(anchor), int(max_bytes), _ip(P) if n else None, n, _dp(R),
                                         _dp(t), _dp(info), _dp(joint), _dp(rel), _dp(gate), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_ml_pair_gate failed (a robust-loss group, a group that does not host every node, a graph "
                               "that is not the group's, an anchor or a pair outside it, or an information matrix -- the graph's or "
                               "a candidate's -- that is not symmetric positive definite)")
        return pairs_output(joint, rel, gate, r, True, threshold)

    def ml_hessian(self, X, anchor=0, graph=None):
        """Debug: the anchored Gauss-Newton Hessian of F_ml as the device wrote it (dpgo_group_ml_hessian).  Returns (ptr,
        col, val, g, F): the CSR of `cov_hessian`, the tangent gradient (dof N by global pose, zeros on the anchor), F_ml."""
        X, ld = _fcol(X)
        n = _dof(self.d) * self.graph.num_poses
        args = (self._h, (graph or self.graph)._h, _dp(X), ld, int(anchor))
        g, F = np.zeros(n), C.c_double(0)
        ptr, col, val = _csr_out(n, "dpgo_group_ml_hessian", lambda *csr: lib().dpgo_group_ml_hessian(*args, *csr, None, None),
                                 lambda *csr: lib().dpgo_group_ml_hessian(*args, *csr, _dp(g), C.byref(F)))
        return ptr, col, val, g, F.value

    def ml_hessian_guarded(self, X, nnz, anchor=0, graph=None, pad=64, sentinel=-7.25e-300):
        """Debug: k_ml_hessian on a sentinel-padded array of the call's own (dpgo_group_debug_ml_hessian_guarded).  nnz: the
        length of `ml_hessian`'s val.  Returns (guards (2, pad) as the device left them, val in `ml_hessian`'s order)."""
        X, ld = _fcol(X)
        guards, val = np.zeros((2, int(pad))), np.zeros(int(nnz))
        if lib().dpgo_group_debug_ml_hessian_guarded(self._h, (graph or self.graph)._h, _dp(X), ld, int(anchor), int(pad),
                                                     float(sentinel), _dp(guards), _dp(val), len(val)) != 0:
            raise RuntimeError("dpgo_group_debug_ml_hessian_guarded failed")
        return guards, val

    def ml_eval(self, X, graph=None, full=False):
        """F_ml and the per-edge residuals at X on the device (dpgo_group_ml_eval).  Returns (F, r (m, dof), chi2 (m),
        near_pi): chi2_e = r_e' Omega_e r_e, F = 1/2 sum chi2 in the device's order of summation.  full=True (debug): a fifth
        item, the dict of what else the edge pass left on the device -- wr (m, dof), grad (m, 2, dof), Ji, Jj, Wi, Wj (m, dof,
        dof; W = Omega J)."""
        X, ld = _fcol(X)
        g_ = graph or self.graph
        F, near = C.c_double(0), C.c_longlong(0)
        dof = _dof(self.d)
        r, chi2 = np.zeros((g_.num_edges, dof)), np.zeros(g_.num_edges)
        wr, grad, jw = np.zeros((g_.num_edges, dof)), np.zeros((g_.num_edges, 2, dof)), np.zeros((g_.num_edges, 4, dof, dof))
        more = (_dp(wr), _dp(grad), _dp(jw)) if full else (None, None, None)
        if lib().dpgo_group_ml_eval(self._h, g_._h, _dp(X), ld, C.byref(F), C.byref(near), _dp(r), _dp(chi2), *more) != 0:
            raise RuntimeError("dpgo_group_ml_eval failed (a robust-loss group, a group that does not host every node, a graph that "
                               "is not the group's, or an information matrix that is not symmetric positive definite)")
        out = (F.value, r, chi2, near.value)
        return out + (dict(wr=wr, grad=grad, Ji=jw[:, 0], Jj=jw[:, 1], Wi=jw[:, 2], Wj=jw[:, 3]),) if full else out

    def ml_gnc(self, graph, X, opt=None, robust_set=None, max_bytes=0):
        """Graduated non-convexity on the full information matrices (dpgo_group_ml_gnc): `gnc`'s levels on chi2_e =
        r_e' Omega_e r_e of `ml_polish`'s objective, so that opt.barc2 is a chi2_dof quantile (dof 3 for d = 2, 6 for d = 3:
        16.266 / 22.458 at 0.999) whatever the noise of an edge.  The robust set is the inter-node edges of `graph`, or the
        edges with robust_set[e] != 0.  Every level solves the weighted problem with `ml_polish`'s loop; an inner MAX_STEPS
        is normal (Gauss-Newton converges linearly while the weighted residuals are large) and only an inner STALLED fails the
        call's level.  An edge of weight exactly 0 contributes exact zeros by selection.  opt: GncOptions (None: the
        defaults).  Returns (Xout, weights, MlGncResult, log) as `gnc` does, F and s on chi2; result.near_pi counts the
        edges with w > 0 whose rotation residual is within 1e-3 of pi at the final point, near_pi_all every such edge."""
        return self._gnc_call("ml_gnc", MlGncResult(), graph, X, opt, robust_set, max_bytes,
                              "an information matrix that is not symmetric positive definite, a bad kind, barc2, mu_step, "
                              "max_levels or anchor")

    def ml_gnc_eval(self, graph, X, kind, mu, barc2, robust_set=None, w_in=None, w_start=None, full=False):
        """Debug: one edge pass of `ml_gnc` at X (dpgo_group_ml_gnc_eval).  w_in None: WEIGH -- the weight array starts as
        w_start (default: ones) and weight_mu(chi2_e) is written on the robust set; otherwise FIXED on w_in.  Returns (chi2, w,
        sums): chi2 unweighted, w the array behind the pass, sums = (sum_{not R} chi2, sum_R w chi2, sum_R rho_mu(chi2),
        max_R chi2, min_R w, the counts of w == 0, w == 1, 0 < w < 1 over R, near_pi over w > 0, near_pi over every edge).
        full=True: a fourth item, the dict of what else the pass left on the device -- r, wr = w Omega r (m, dof), grad (m, 2,
        dof), Ji, Jj, Wi, Wj (m, dof, dof; W = w Omega J; all four zero where w == 0)."""
        m, dof = graph.num_edges, _dof(self.d)
        head, w = self._gnc_eval_args("ml_gnc_eval", graph, X, kind, mu, barc2, robust_set, w_in, w_start)
        chi2, sums = np.zeros(m), np.zeros(10)
        r, wr, grad, jw = np.zeros((m, dof)), np.zeros((m, dof)), np.zeros((m, 2, dof)), np.zeros((m, 4, dof, dof))
        more = (_dp(r), _dp(wr), _dp(grad), _dp(jw)) if full else (None,) * 4
        if lib().dpgo_group_ml_gnc_eval(*head, int(bool(full)), _dp(chi2), _dp(w), _dp(sums), *more) != 0:
            raise RuntimeError("dpgo_group_ml_gnc_eval failed (a robust-loss group, a group that does not host every node, a graph "
                               "that is not the group's, an information matrix that is not symmetric positive definite, a bad "
                               "kind, mu or barc2, or bad sizes)")
        out = (chi2, w, sums)
        return out + (dict(r=r, wr=wr, grad=grad, Ji=jw[:, 0], Jj=jw[:, 1], Wi=jw[:, 2], Wj=jw[:, 3]),) if full else out

    def ml_gnc_hessian(self, graph, X, w, robust_set=None, anchor=0):
        """Debug: the weighted gradient g_w and the anchored Gauss-Newton Hessian H_w of `ml_gnc` for the given weights as
        the device wrote them (dpgo_group_debug_ml_gnc_hessian).  Returns (ptr, col, val, g) as `ml_hessian` does."""
        X, ld = _fcol(X)
        n = _dof(self.d) * self.graph.num_poses
        rs = None if robust_set is None else np.ascontiguousarray(robust_set, np.int32)
        wi = np.ascontiguousarray(w, np.float64)
        if wi.shape != (graph.num_edges,) or (rs is not None and rs.shape != wi.shape):
            raise ValueError("ml_gnc_hessian: w and robust_set must have one entry per edge")
        args = (self._h, graph._h, _dp(X), ld, int(anchor), None if rs is None else _ip(rs), _dp(wi))
        g = np.zeros(n)
        ptr, col, val = _csr_out(n, "dpgo_group_debug_ml_gnc_hessian",
                                 lambda *csr: lib().dpgo_group_debug_ml_gnc_hessian(*args, *csr, None),
                                 lambda *csr: lib().dpgo_group_debug_ml_gnc_hessian(*args, *csr, _dp(g)))
        return ptr, col, val, g

    def robust_matrix(self, X, loss, loss_reg=0.25, graph=None):
        """Debug: M_w = sum_e w_e(X) M_e as the device wrote it (dpgo_group_robust_matrix): CSR as `cert_matrix` hands out S."""
        X, ld = _fcol(X)
        args = (self._h, (graph or self.graph)._h, _dp(X), ld, int(loss), float(loss_reg))
        return _csr_out((self.d + 1) * self.graph.num_poses, "dpgo_group_robust_matrix",
                        lambda *csr: lib().dpgo_group_robust_matrix(*args, *csr))

    def staircase(self, X, max_bytes=0, **opts):
        """The Riemannian staircase (dpgo_group_staircase): from X -- usually a point whose certificate is NEGATIVE -- TNT at
        rank r, verify at Lambda(Y), an escape along the certificate's direction one rank up, until the certificate is not
        NEGATIVE or r = r_max <= 2d; then the rounding back to SO(d)^N and a polish.  Trivial-loss groups that host every
        node.  opts: the fields of StaircaseOptions.  Returns (Xhat, StaircaseResult, log, Y): the result (X itself for
        STAIR_SKIPPED; never worse than X), the result struct, one row per level of (rank, F in, F out, |grad|, TNT iterations,
        Hessian products, certificate status, theta, accepted alpha, halvings), and the final lifted point (d+1)N x 2d.
        result.gap = F_final - F_sdp bounds the distance to the global minimum only where cert_status is CERT_PROVEN and
        stationarity is small.  The optimiser's state is not touched."""
        X, ld = _fcol(X)
        o = StaircaseOptions(**opts)
        Xhat = np.array(X, order="F")
        Y = np.zeros((X.shape[0], 2 * self.d), order="F")
        log = np.zeros((self.d + 1, 10))
        r = StaircaseResult()
        if lib().dpgo_group_staircase(self._h, _dp(X), ld, C.byref(o), int(max_bytes), _dp(Xhat), Xhat.shape[0], _dp(Y), Y.shape[0],
                                      _dp(log), len(log), C.byref(r)) != 0:
            raise RuntimeError("dpgo_group_staircase failed (robust loss, a group that does not host every node, r_max outside "
                               "[d, 2d], or bad sizes or options)")
        return Xhat, r, log[:min(len(log), r.levels)].copy(), Y

    def _lifted(self, Y, what):
        Y, ld = _fcol(Y)
        if Y.shape[1] != 2 * self.d:
            raise ValueError("%s: a lifted point is (d+1)N x 2d" % what)
        return Y, ld

    def stair_eval(self, Y):
        """Debug: (F, |grad F|, Lambda (N, d, d), grad = S Y) at the lifted point Y, (d+1)N x 2d with zero columns >= r."""
        Y, ld = self._lifted(Y, "stair_eval")
        N = Y.shape[0] // (self.d + 1)
        F, gn = C.c_double(0), C.c_double(0)
        Lam, G = np.zeros((N, self.d, self.d)), np.zeros(Y.shape, order="F")
        if lib().dpgo_group_stair_eval(self._h, _dp(Y), ld, C.byref(F), C.byref(gn), _dp(Lam), _dp(G), G.shape[0]) != 0:
            raise RuntimeError("dpgo_group_stair_eval failed")
        return F.value, gn.value, Lam, G

    def stair_hess(self, Y, V):
        """Debug: Hess[V] = Proj_Y(S(Y) V) at the lifted point Y."""
        Y, ld = self._lifted(Y, "stair_hess")
        V, ldv = self._lifted(V, "stair_hess")
        out = np.zeros(Y.shape, order="F")
        if lib().dpgo_group_stair_hess(self._h, _dp(Y), ld, _dp(V), ldv, _dp(out), out.shape[0]) != 0:
            raise RuntimeError("dpgo_group_stair_hess failed")
        return out

    def stair_retract(self, Y, V):
        """Debug: the polar retraction of Y + V."""
        Y, ld = self._lifted(Y, "stair_retract")
        V, ldv = self._lifted(V, "stair_retract")
        Z = np.zeros(Y.shape, order="F")
        if lib().dpgo_group_stair_retract(self._h, _dp(Y), ld, _dp(V), ldv, _dp(Z), Z.shape[0]) != 0:
            raise RuntimeError("dpgo_group_stair_retract failed")
        return Z

    def stair_round(self, Y):
        """Debug: the rounding of the lifted point Y: (B (2d, d), the 2d singular values, Xhat before any polish)."""
        Y, ld = self._lifted(Y, "stair_round")
        B, sig, Xh = np.zeros((2 * self.d, self.d)), np.zeros(2 * self.d), np.zeros((Y.shape[0], self.d), order="F")
        if lib().dpgo_group_stair_round(self._h, _dp(Y), ld, _dp(B), _dp(sig), _dp(Xh), Xh.shape[0]) != 0:
            raise RuntimeError("dpgo_group_stair_round failed")
        return B, sig, Xh

    def cov_hessian(self, X, anchor=0):
        """Debug: the matrix covariance factors, the anchored tangent-space Hessian, read back from the device: CSR (ptr, col,
        val) on the unknowns dof g + a of the global poses g, every stored dof x dof block dense, the anchor's row and
        column those of the identity."""
        X, ld = _fcol(X)
        return _csr_out(_dof(self.d) * self.graph.num_poses, "dpgo_group_cov_hessian",
                        lambda *csr: lib().dpgo_group_cov_hessian(self._h, _dp(X), ld, int(anchor), *csr))

    def cert_lambda(self, X):
        """compute_Lambda_blocks (SESyncProblem.cpp:375-395): the N symmetric d x d blocks of Lambda(X), (N, d, d)."""
        X, ld = _fcol(X)
        L = np.zeros((self.graph.num_poses, self.d, self.d))
        if lib().dpgo_group_cert_lambda(self._h, _dp(X), ld, _dp(L)) != 0:
            raise RuntimeError("dpgo_group_cert_lambda failed")
        return L

    def cert_apply(self, X, V):
        """S(X) V for a block V of the shape of X (the operator of verify_solution alone)."""
        X, ld = _fcol(X)
        V = np.asarray(V)
        if V.shape != X.shape:
            raise ValueError("cert_apply: V must have the shape of X, %r" % (X.shape,))
        V, ldv = _fcol(V)
        SV = np.zeros_like(X, order="F")
        if lib().dpgo_group_cert_apply(self._h, _dp(X), ld, _dp(V), ldv, _dp(SV), SV.shape[0]) != 0:
            raise RuntimeError("dpgo_group_cert_apply failed")
        return SV

    def set_options(self, options):
        rc = lib().dpgo_group_set_options(self._h, C.byref(options))
        if rc == 0:
            self.options = options
        return rc

    def get_options(self):
        o = Options()
        lib().dpgo_group_get_options(self._h, C.byref(o))
        return o

    def results(self, k):
        r = Results()
        lib().dpgo_group_results(self._h, k, C.byref(r))
        return r

    def solver_stats(self):
        a, b, c, d = C.c_long(), C.c_long(), C.c_int(), C.c_int()
        lib().dpgo_group_solver_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return dict(nnz_tt=a.value, nnz_rr=b.value, levels_tt=c.value, levels_rr=d.value)

    def graph_stats(self):
        """Segments of the iteration replayed from captured graphs, graphs captured, segments launched eagerly."""
        a, b, c = C.c_long(), C.c_long(), C.c_long()
        lib().dpgo_group_graph_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return dict(replays=a.value, captures=b.value, eager=c.value)

    def debug_apply(self, k, op, X, out_rows):
        X, ld = _fcol(X)
        out = np.zeros((out_rows, self.d), order="F")
        if lib().dpgo_group_debug_apply(self._h, k, op.encode(), _dp(X), ld, _dp(out), out.shape[0]) != 0:
            raise RuntimeError("debug_apply(%s) failed" % op)
        return out


    def debug_stpcg(self, locals_, YG, Delta, device_start, fill=0.0):
        """Debug: one truncated CG of a refinement round on given points (dpgo_group_debug_stpcg).  locals_: the nodes that
        take part; YG: per node of the group (all of them) the stacked [Y ; g], 2 (d+1) n0 x d; Delta: one radius per node of
        the group; device_start: the first round's start (True) or a later round's (False).  Returns a list with one dict per
        node of the group: s, hs, grad ((d+1) n0 x d each; `fill` everywhere for a node outside locals_), sums (6), h_M_norm,
        cg_it, stop_ord, active, live, Delta."""
        L, d = len(self.node_ids), self.d
        rows = [(d + 1) * self.sizes[a][0] for a in range(L)]
        if len(YG) != L or any(np.shape(YG[a]) != (2 * rows[a], d) for a in range(L)):
            raise ValueError("debug_stpcg: one [Y ; g] of 2 (d+1) n0 rows per node of the group")
        X = np.asfortranarray(np.vstack([np.asarray(m, np.float64) for m in YG]))
        out = np.zeros((3 * sum(rows), d), order="F")
        sc = np.zeros((L, 12))
        ids = np.asarray(list(locals_), np.int32)
        Dl = np.ascontiguousarray(np.asarray(Delta, np.float64))
        if Dl.shape != (L,):
            raise ValueError("debug_stpcg: one radius per node of the group")
        if lib().dpgo_group_debug_stpcg(self._h, _ip(ids), len(ids), _dp(X), X.shape[0], _dp(Dl), int(bool(device_start)),
                                        float(fill), _dp(out), out.shape[0], _dp(sc)) != 0:
            raise RuntimeError("dpgo_group_debug_stpcg failed")
        res, r0 = [], 0
        for a in range(L):
            R0 = rows[a]
            res.append(dict(s=out[r0:r0 + R0].copy(), hs=out[r0 + R0:r0 + 2 * R0].copy(), grad=out[r0 + 2 * R0:r0 + 3 * R0].copy(),
                            sums=sc[a, :6].copy(), h_M_norm=float(sc[a, 6]), cg_it=int(sc[a, 7]), stop_ord=int(sc[a, 8]),
                            active=int(sc[a, 9]), live=int(sc[a, 10]), Delta=float(sc[a, 11])))
            r0 += 3 * R0
        return res

    def _mat(self, X, rows, what):
        """A reference-layout operand as a Fortran-contiguous float64 matrix of exactly `rows` rows (kept alive by the caller)."""
        X = np.asfortranarray(np.asarray(X, np.float64))
        if X.shape != (rows, self.d):
            raise ValueError("%s: %d x %d expected, got %s" % (what, rows, self.d, X.shape))
        return X

    def debug_edge_offsets(self):
        """Debug: first inter-node edge of every node of the group among the group's edges (len(node_ids) + 1 entries)."""
        o = np.zeros(len(self.node_ids) + 1, np.int32)
        if lib().dpgo_group_debug_edge_offsets(self._h, _ip(o)) != 0:
            raise RuntimeError("dpgo_group_debug_edge_offsets failed")
        return o

    def debug_inter_update(self, k, Z, Zprev=None, DfE_old=None, GX=None, X=None, Znbr=None, recv=None, nsrc=None, whole=False,
                           sentinel=None, fused_Df=True):
        """Debug: update()'s inter-edge pass of node k at Z (dpgo_group_debug_inter_update; robust losses).  Z, Zprev, DfE_old,
        Znbr: (d+1)(n0+n1) x d, reference layout; GX, X: (d+1) n0 x d.  Zprev and DfE_old: the quad term; GX and X: the fused
        Dfobj (fused_Df=False: by the launch of its own behind the pass); Znbr: the halo copy -- Z's neighbour rows are then pre-filled with `sentinel` (if given) since the pass must not
        read them; recv ((d+1) nrecv x d) and nsrc (n1 slots, -1: not delivered): the lazy unpack.  Returns a dict: DfE, g, w,
        sums (slots 0..4), Df (with GX), Z_after, Znbr_after."""
        d = self.d
        n0, n1 = self.sizes[k][0], self.sizes[k][1]
        own, all_ = (d + 1) * n0, (d + 1) * (n0 + n1)
        q, keep = InterUpdateDebug(), []

        def put(name, M, rows):
            if M is None:
                return
            M = self._mat(M, rows, name)
            keep.append(M)
            setattr(q, name, _dp(M))

        Z = np.array(Z, np.float64, order="F")
        if Znbr is not None and sentinel is not None:
            Z[own:] = sentinel
        q.local, q.whole, q.quad, q.with_Df = k, int(bool(whole)), int(Zprev is not None), (0 if GX is None else (1 if fused_Df else 2))
        put("Z", Z, all_); put("Zprev", Zprev, all_); put("DfE_old", DfE_old, all_); put("Znbr", Znbr, all_)
        put("GX", GX, own); put("X", X, own)
        if recv is not None:
            recv = np.asfortranarray(np.asarray(recv, np.float64))
            q.nrecv = recv.shape[0] // (d + 1)
            put("recv", recv, (d + 1) * q.nrecv)
            ns = np.ascontiguousarray(np.asarray(nsrc, np.int32))
            if ns.shape != (n1,):
                raise ValueError("nsrc: one slot per neighbour row")
            keep.append(ns)
            q.nsrc = _ip(ns)
        m1 = int(np.diff(self.debug_edge_offsets())[k])
        out = dict(DfE=np.zeros((all_, d), order="F"), g=np.zeros((own, d), order="F"), w=np.zeros(max(m1, 1)), sums=np.zeros(5),
                   Df=np.zeros((own, d), order="F"), Z_after=np.zeros((all_, d), order="F"), Znbr_after=np.zeros((all_, d), order="F"))
        for name, M in out.items():
            setattr(q, name, _dp(M))
        if lib().dpgo_group_debug_inter_update(self._h, C.byref(q)) != 0:
            raise RuntimeError("dpgo_group_debug_inter_update failed")
        out["w"] = out["w"][:m1]
        if GX is None:
            del out["Df"]
        return out

    def debug_inter_iterate(self, k, Zc, Zp, gamma, GXc=None, GXp=None, Xref=None, fused=True, prox=False, gamma_dev=False,
                            whole=False):
        """Debug: iterate()'s inter-edge pass of node k at Y = Zc + gamma[k] (Zc - Zp) (dpgo_group_debug_inter_iterate), enqueued as
        the iteration enqueues it.  gamma: one per node of the group; GXc, GXp: the kept products (a statically scaled group needs
        them); prox (with Xref): the proximal half step.  Returns a dict: Y, g, Df, sums (<Y, g>, |Xout - Xref|^2), Xout, Xref."""
        d = self.d
        n0, n1 = self.sizes[k][0], self.sizes[k][1]
        own, all_ = (d + 1) * n0, (d + 1) * (n0 + n1)
        q, keep = InterIterateDebug(), []
        q.local, q.whole, q.fused, q.prox, q.gamma_dev = k, int(bool(whole)), int(bool(fused)), int(bool(prox)), int(bool(gamma_dev))
        for name, M, rows in (("Zc", Zc, all_), ("Zp", Zp, all_), ("GXc", GXc, own), ("GXp", GXp, own), ("Xref", Xref, own)):
            if M is not None:
                M = self._mat(M, rows, name)
                keep.append(M)
                setattr(q, name, _dp(M))
        gam = np.ascontiguousarray(np.asarray(gamma, np.float64))
        if gam.shape != (len(self.node_ids),):
            raise ValueError("gamma: one per node of the group")
        q.gamma = _dp(gam)
        out = dict(Y=np.zeros((all_, d), order="F"), g=np.zeros((own, d), order="F"), Df=np.zeros((own, d), order="F"),
                   Xout=np.zeros((own, d), order="F"), Xref_after=np.zeros((own, d), order="F"), sums=np.zeros(2))
        for name, M in out.items():
            setattr(q, name, _dp(M))
        if lib().dpgo_group_debug_inter_iterate(self._h, C.byref(q)) != 0:
            raise RuntimeError("dpgo_group_debug_inter_iterate failed")
        return out

    def debug_cost(self, k, Z, eform=False, whole=False):
        """Debug: k_cost's two slots of node k at Z ((d+1)(n0+n1) x d): (intra-node edges' costs, inter-node edges' rho)."""
        n0, n1 = self.sizes[k][0], self.sizes[k][1]
        Z = self._mat(Z, (self.d + 1) * (n0 + n1), "Z")
        sums = np.zeros(2)
        if lib().dpgo_group_debug_cost(self._h, k, int(bool(whole)), int(bool(eform)), _dp(Z), _dp(sums)) != 0:
            raise RuntimeError("dpgo_group_debug_cost failed")
        return sums

    def debug_rescale(self, w, scale, count, max_rescale_count, nodes):
        """Debug: the Dynamic rescale's test on given edge weights, scales (one per inter-node edge of the group:
        debug_edge_offsets) and counters (one per node), over the node set `nodes`, then the rescale of the flagged nodes
        (dpgo_group_debug_rescale).  Returns a dict: rescaled (how many), flags, host_flags, scale, count."""
        L = len(self.node_ids)
        m = int(self.debug_edge_offsets()[-1])
        w = np.ascontiguousarray(np.asarray(w, np.float64))
        scale = np.ascontiguousarray(np.asarray(scale, np.float64))
        count = np.ascontiguousarray(np.asarray(count, np.int32))
        nodes = np.ascontiguousarray(np.asarray(list(nodes), np.int32))
        if w.shape != (m,) or scale.shape != (m,) or count.shape != (L,):
            raise ValueError("debug_rescale: one weight and scale per inter-node edge of the group, one counter per node")
        flags, hf, so, co = np.zeros(L, np.int32), np.zeros(L), np.zeros(max(m, 1)), np.zeros(L, np.int32)
        n = lib().dpgo_group_debug_rescale(self._h, _dp(w), _dp(scale), _ip(count), int(max_rescale_count), _ip(nodes), len(nodes),
                                           _ip(flags), _dp(hf), _dp(so), _ip(co))
        if n < 0:
            raise RuntimeError("dpgo_group_debug_rescale failed")
        return dict(rescaled=n, flags=flags, host_flags=hf, scale=so[:m], count=co)

    def _cert_blocks(self, names, mats):
        rows = (self.d + 1) * self.graph.num_poses
        out = []
        for name, M in zip(names, mats):
            M = np.asfortranarray(np.asarray(M, np.float64))
            if M.shape != (rows, self.d):
                raise ValueError("%s must be %r" % (name, (rows, self.d)))
            out.append(M)
        return rows, out

    def debug_cert_gram(self, X, V, W, P, SV, SP, MW=None):
        """Debug: one launch of k_cert_gram and one of k_cert_reduce on given blocks, as the certificate's search makes them
        (dpgo_group_debug_cert_gram).  Lambda is that of X; the buffer of S W takes MW (= M W), or with MW None the product
        M W the loop forms.  Returns (sums, SW): the raw host sums -- the upper triangles of B^T B and of B^T (S B), row-major,
        then 2 d slots the launch does not write -- and the finished S W."""
        rows, (X, V, W, P, SV, SP) = self._cert_blocks(("X", "V", "W", "P", "SV", "SP"), (X, V, W, P, SV, SP))
        mw = None
        if MW is not None:
            MW = self._cert_blocks(("MW",), (MW,))[1][0]
            mw = _dp(MW)
        d = self.d
        sums, SW = np.zeros(3 * d * (3 * d + 1) + 2 * d), np.zeros((rows, d), order="F")
        if lib().dpgo_group_debug_cert_gram(self._h, _dp(X), _dp(V), _dp(W), _dp(P), _dp(SV), _dp(SP), mw, rows, _dp(sums), _dp(SW)) != 0:
            raise RuntimeError("dpgo_group_debug_cert_gram failed")
        return sums, SW

    def debug_cert_update(self, C_, theta, V, W, P, SV, SW, SP, precondition, nbr_fill=0.0):
        """Debug: one launch of k_cert_update and one of k_cert_reduce on given blocks (dpgo_group_debug_cert_update).  C_: 3d x d
        (the rows of V, W, P), theta: d.  Returns a dict: V, W, P, SV, SW, SP (the buffers afterwards), rr, vv (the launch's
        sums |R'_j|^2, |V'_j|^2) and nbr ((3, P1, (d+1) d): the neighbour records of V, W, P, which were nbr_fill before)."""
        d = self.d
        rows, ins = self._cert_blocks(("V", "W", "P", "SV", "SW", "SP"), (V, W, P, SV, SW, SP))
        Cm = np.ascontiguousarray(np.asarray(C_, np.float64))
        th = np.ascontiguousarray(np.asarray(theta, np.float64))
        if Cm.shape != (3 * d, d) or th.shape != (d,):
            raise ValueError("debug_cert_update: C is 3d x d, theta has d entries")
        p1 = lib().dpgo_group_debug_cert_nbr_rows(self._h)
        out = dict((k, np.zeros((rows, d), order="F")) for k in ("V", "W", "P", "SV", "SW", "SP"))
        sums, nbr = np.zeros(3 * d * (3 * d + 1) + 2 * d), np.zeros((3, max(p1, 0), (d + 1) * d))
        q = CertUpdateDebug()
        q.C, q.theta = _dp(Cm), _dp(th)
        for k, M in zip(("V", "W", "P", "SV", "SW", "SP"), ins):
            setattr(q, k, _dp(M))
            setattr(q, k + "_out", _dp(out[k]))
        q.ld, q.precondition, q.nbr_fill, q.sums, q.nbr = rows, int(bool(precondition)), float(nbr_fill), _dp(sums), _dp(nbr)
        if lib().dpgo_group_debug_cert_update(self._h, C.byref(q)) != 0:
            raise RuntimeError("dpgo_group_debug_cert_update failed")
        nt2 = 3 * d * (3 * d + 1)
        out.update(rr=sums[nt2:nt2 + d].copy(), vv=sums[nt2 + d:].copy(), nbr=nbr)
        return out

    def debug_cert_precon(self):
        """Debug: the block-Jacobi blocks T_p the certificate's search applies, (N, d+1, d+1) by global pose."""
        T = np.zeros((self.graph.num_poses, self.d + 1, self.d + 1))
        if lib().dpgo_group_debug_cert_precon(self._h, _dp(T)) != 0:
            raise RuntimeError("dpgo_group_debug_cert_precon failed")
        return T

    def debug_cert_trace(self, on):
        """Debug: switch the trace of the certificate's search on or off (off is the default)."""
        if lib().dpgo_group_debug_cert_trace(self._h, int(bool(on))) != 0:
            raise RuntimeError("dpgo_group_debug_cert_trace failed")

    def debug_cert_trace_get(self):
        """Debug: the passes of the last traced search, a list of dicts: sums, nblk, used, theta (d), C (3d x d), refresh."""
        d = self.d
        ln, cnt = C.c_int(0), C.c_longlong(0)
        if lib().dpgo_group_debug_cert_trace_get(self._h, None, 0, C.byref(ln), C.byref(cnt)) != 0:
            raise RuntimeError("dpgo_group_debug_cert_trace_get failed")
        rec = np.zeros((cnt.value, ln.value))
        if cnt.value and lib().dpgo_group_debug_cert_trace_get(self._h, _dp(rec), rec.size, C.byref(ln), C.byref(cnt)) != 0:
            raise RuntimeError("dpgo_group_debug_cert_trace_get failed")
        ns = 3 * d * (3 * d + 1) + 2 * d
        return [dict(sums=r[:ns].copy(), nblk=int(r[ns]), used=int(r[ns + 1]), theta=r[ns + 2:ns + 2 + d].copy(),
                     C=r[ns + 2 + d:ns + 2 + d + 3 * d * d].reshape(3 * d, d).copy(), refresh=bool(r[-1])) for r in rec]

    def debug_seg_layout(self):
        """Debug: (nseg_all, own_ptr, nbr_ptr) -- the segment table the partial sums are laid out by: node a's own segments
        are [own_ptr[a], own_ptr[a+1]), its neighbour segments [nbr_ptr[a], nbr_ptr[a+1])."""
        L = len(self.node_ids)
        n, own, nbr = C.c_int(0), np.zeros(L + 1, np.int32), np.zeros(L + 1, np.int32)
        if lib().dpgo_group_debug_seg_layout(self._h, C.byref(n), _ip(own), _ip(nbr)) != 0:
            raise RuntimeError("dpgo_group_debug_seg_layout failed")
        return n.value, own, nbr

    def debug_cg_scalars(self, script):
        """Debug: the scalar kernels of the truncated CG on given partial sums (dpgo_group_debug_cg_scalars).  script: a list
        of dicts, each one launch: kind ("begin_host", "begin_device", "scal0", "scal1", "scal_begin"); bits, max_it, Delta
        (per node) for the begin kinds; rv, target (per node) for begin_host; use_precon, grad_tol, pgrad_tol, kappa, theta
        for begin_device and scal_begin; partials (slots, nseg_all), optional.  kind "reduce_gate": the trial point's
        reduction with the gate of a speculative update, gate = dict(nslots, GATE_OPTIONS, GATE_NODE_SCALARS per node); kind
        "reduce": the plain own-row reduction of gate["nslots"] sums.  Returns one dict per launch: records (a
        list of dicts with CG_RECORD_FIELDS, the four counters as ints), masks (three ints), cg_summary (L, 3), tnt_summary
        and dev_tnt (L, 7), flag (the host flag's value), seq (the last sequence number given out), arrived; after a
        reduce_gate or a reduce also host_scalars and dev_sums (L, MAX_SLOTS), go (the gate's word) and h_gate (its pinned
        verdict)."""
        L, n = len(self.node_ids), len(script)
        nseg_all = self.debug_seg_layout()[0]
        arr, keep = (CgDebugLaunch * max(n, 1))(), []

        def per_node(q, key, dtype=np.float64, ptr=_DP):
            v = np.ascontiguousarray(np.asarray(q.get(key, np.zeros(L)), dtype))
            if v.shape != (L,):
                raise ValueError("debug_cg_scalars: %s takes one value per node" % key)
            keep.append(v)
            return v.ctypes.data_as(ptr)

        for i, q in enumerate(script):
            a = arr[i]
            a.kind = CG_DEBUG_KINDS.index(q["kind"])
            a.bits, a.use_precon, a.max_it = int(q.get("bits", 0)), int(q.get("use_precon", 0)), int(q.get("max_it", 0))
            a.grad_tol, a.pgrad_tol = float(q.get("grad_tol", 0.0)), float(q.get("pgrad_tol", 0.0))
            a.kappa, a.theta = float(q.get("kappa", 0.0)), float(q.get("theta", 0.0))
            a.rv, a.Delta, a.target = per_node(q, "rv"), per_node(q, "Delta"), per_node(q, "target")
            a.slots, a.partials, a.gate = 0, None, None
            if q.get("partials") is not None:
                P = np.ascontiguousarray(np.asarray(q["partials"], np.float64))
                if P.ndim != 2 or P.shape[1] != nseg_all:
                    raise ValueError("debug_cg_scalars: partials are (slots, nseg_all = %d)" % nseg_all)
                keep.append(P)
                a.slots, a.partials = P.shape[0], P.ctypes.data_as(_DP)
            if q.get("gate") is not None:
                g, G = q["gate"], GateDebug()
                G.nslots = int(g["nslots"])
                for k in GATE_OPTIONS:
                    setattr(G, k, g.get(k, 0))
                if q["kind"] == "reduce_gate":
                    for k in GATE_NODE_SCALARS:
                        ints = k.startswith("hits")
                        setattr(G, k, per_node(g, k, np.int32 if ints else np.float64, _IP if ints else _DP))
                keep.append(G)
                a.gate = C.addressof(G)
        nf = len(CG_RECORD_FIELDS)
        rec, masks = np.zeros((n, L, nf)), np.zeros((n, 3), np.uint64)
        cgs, tnt, dev = np.zeros((n, L, 4)), np.zeros((n, L, 8)), np.zeros((n, L, 8))
        seq, arrived = np.zeros((n, 2), np.uint64), np.zeros(n, np.uint32)
        gsums, gwords = np.zeros((n, 2, L, MAX_SLOTS)), np.zeros((n, 2), np.uint64)
        _ULP = C.POINTER(C.c_ulonglong)
        if lib().dpgo_group_debug_cg_scalars(self._h, arr, n, _dp(rec), masks.ctypes.data_as(_ULP), _dp(cgs),
                                             _dp(tnt), _dp(dev), seq.ctypes.data_as(_ULP),
                                             arrived.ctypes.data_as(C.POINTER(C.c_uint)), _dp(gsums), gwords.ctypes.data_as(_ULP)) != 0:
            raise RuntimeError("dpgo_group_debug_cg_scalars failed")
        out = []
        for i in range(n):
            records = [{f: (int(rec[i, a, k]) if k >= nf - 4 else float(rec[i, a, k])) for k, f in enumerate(CG_RECORD_FIELDS)}
                       for a in range(L)]
            out.append(dict(records=records, masks=[int(m) for m in masks[i]], cg_summary=cgs[i, :, :3].copy(),
                            tnt_summary=tnt[i, :, :7].copy(), dev_tnt=dev[i, :, :7].copy(), flag=int(seq[i, 0]), seq=int(seq[i, 1]),
                            arrived=int(arrived[i])))
            if script[i]["kind"] in ("reduce_gate", "reduce"):
                out[-1].update(host_scalars=gsums[i, 0].copy(), dev_sums=gsums[i, 1].copy(), go=int(gwords[i, 0]),
                               h_gate=float(gwords[i, 1:2].view(np.float64)[0]))
        return out

    def debug_star_sums(self, partials, valid):
        """Debug: AMM-PGO*'s master sums on given partial sums (dpgo_group_debug_star_sums).  partials: (MAX_SLOTS, nseg_all);
        valid: bit q = sum q was produced.  Returns dict(dev (4), host (4), flag, seq)."""
        nseg_all = self.debug_seg_layout()[0]
        P = np.ascontiguousarray(np.asarray(partials, np.float64))
        if P.shape != (MAX_SLOTS, nseg_all):
            raise ValueError("debug_star_sums: partials are (%d, nseg_all = %d)" % (MAX_SLOTS, nseg_all))
        out, seq = np.zeros(8), np.zeros(2, np.uint64)
        if lib().dpgo_group_debug_star_sums(self._h, _dp(P), int(valid), _dp(out), seq.ctypes.data_as(C.POINTER(C.c_ulonglong))) != 0:
            raise RuntimeError("dpgo_group_debug_star_sums failed")
        return dict(dev=out[:4].copy(), host=out[4:].copy(), flag=int(seq[0]), seq=int(seq[1]))

    def debug_gated_update(self, go_word):
        """Debug: the launches of an update enqueued ahead of the host's decision under the gate word go_word, 0 or all ones
        (dpgo_group_debug_gated_update); the group's state is put back afterwards.  Returns {buffer: dict(untouched,
        same_as_ungated)} for the buffers of GATED_BUFFERS the group has; same_as_ungated is None for go_word = 0."""
        rep = np.full(3 * len(GATED_BUFFERS), -7, np.int32)
        if lib().dpgo_group_debug_gated_update(self._h, int(go_word) & 0xFFFFFFFFFFFFFFFF, _ip(rep)) != 0:
            raise RuntimeError("dpgo_group_debug_gated_update failed")
        return {k: dict(untouched=bool(rep[3 * i + 1]), same_as_ungated=None if rep[3 * i + 2] < 0 else bool(rep[3 * i + 2]))
                for i, k in enumerate(GATED_BUFFERS) if rep[3 * i]}


class Comm:
    """The RCCL communicator of one group (one process per GPU): dpgo_comm_* of include/dpgo_amd.h.  `bcast`
    carries the 128-byte unique id from rank 0 to the others: a function bytes -> bytes (e.g. through
    torch.distributed's gloo store, MPI, a file); with one rank it is not needed."""

    def __init__(self, group, rank, nranks, bcast=None):
        self.group, self.rank, self.nranks = group, rank, nranks
        if nranks > 1 and bcast is None:
            raise ValueError("nranks > 1 needs a broadcast function for the unique id")
        idb = C.create_string_buffer(128)
        raw = b""
        if rank == 0 and lib().dpgo_comm_unique_id(idb) == 0:
            raw = bytes(idb.raw)
        if nranks > 1:
            raw = bcast(raw)          # (an empty id tells every rank that rank 0 could not get one: nobody is left waiting)
        if len(raw) != 128:
            raise RuntimeError("dpgo_comm_unique_id failed (RCCL not available)")
        idb = C.create_string_buffer(raw, 128)
        h = C.c_void_p()
        if lib().dpgo_comm_create(group._h, rank, nranks, idb, C.byref(h)) != 0:
            raise RuntimeError("dpgo_comm_create failed")
        self._h = h

    @classmethod
    def self_exchange_only(cls, group):
        """A one-rank communicator that serves exchange() alone, with the rank as its own peer (dpgo_comm_create_self): for a
        group whose neighbours no rank hosts -- one rank of an N-GPU run emulated on one GPU."""
        self = cls.__new__(cls)
        self.group, self.rank, self.nranks = group, 0, 1
        h = C.c_void_p()
        if lib().dpgo_comm_create_self(group._h, C.byref(h)) != 0:
            raise RuntimeError("dpgo_comm_create_self failed")
        self._h = h
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dpgo_comm_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    def exchange(self):
        return lib().dpgo_comm_exchange(self._h)

    def exchange_kind(self):
        """"p2p" (grouped ncclSend / ncclRecv to the real neighbours) or "allgather"."""
        return "p2p" if lib().dpgo_comm_exchange_kind(self._h) == 1 else "allgather"

    def bytes_sent(self):
        """Bytes this rank hands to RCCL per exchange."""
        return int(lib().dpgo_comm_bytes_sent(self._h))

    def self_exchange(self):
        """One rank only: exchange() runs the neighbour-to-neighbour path with this rank as its own peer from now on
        (a measurement mode, dpgo_comm_self_exchange)."""
        if lib().dpgo_comm_self_exchange(self._h) != 0:
            raise RuntimeError("dpgo_comm_self_exchange failed")

    def enable_timing(self):
        if lib().dpgo_comm_enable_timing(self._h) != 0:
            raise RuntimeError("dpgo_comm_enable_timing failed")

    def exchange_time(self):
        """(mean microseconds from 'iterate final' to 'neighbour rows in place', exchanges counted)."""
        us, n = C.c_double(), C.c_long()
        if lib().dpgo_comm_exchange_time(self._h, C.byref(us), C.byref(n)) != 0:
            raise RuntimeError("dpgo_comm_exchange_time failed")
        return us.value, n.value

    def allreduce_sum(self, vals):
        a = np.ascontiguousarray(vals, np.float64).ravel().copy()
        if lib().dpgo_comm_allreduce_sum(self._h, _dp(a), len(a)) != 0:
            raise RuntimeError("dpgo_comm_allreduce_sum failed")
        return a

    def barrier(self):
        return lib().dpgo_comm_barrier(self._h)


class DPGOHash:
    """View of one node of a NodeGroup with the reference's DPGOHash method names
    (C++/DPGO/include/DPGO/DPGOHash.h:13-107)."""

    def __init__(self, group, local):
        self.group, self.local = group, local
        self.node = group.node_ids[local]
        self.n = group.sizes[local][:2]
        self.m = group.sizes[local][2:]
        self.d = group.d

    def initialize(self, X):
        X, ld = _fcol(X)
        if X.shape != ((self.d + 1) * (self.n[0] + self.n[1]), self.d):
            return -1
        return lib().dpgo_group_initialize(self.group._h, self.local, _dp(X), ld)

    def update(self):
        return self.group.update([self.local])

    def iterate(self):
        return self.group.iterate([self.local])

    def results(self):
        return self.group.results(self.local)

    def message_for(self, beta):
        """The message this node owes node beta: ((d+1) |sent[beta]|) x d, [t rows ; R rows]."""
        ns = C.c_int()
        if lib().dpgo_group_message_sizes(self.group._h, self.local, int(beta), C.byref(ns), None) != 0 or ns.value == 0:
            return None
        M = np.zeros(((self.d + 1) * ns.value, self.d), order="F")
        lib().dpgo_group_send(self.group._h, self.local, int(beta), _dp(M), M.shape[0])
        return M

    def receive(self, msg):
        """DPGOHash::receive(const std::map<int, Matrix>&)."""
        rc = 0
        for beta, M in msg.items():
            M, ld = _fcol(M)
            rc |= lib().dpgo_group_receive(self.group._h, self.local, int(beta), _dp(M), ld)
        return rc

    def Xk(self):
        X = np.zeros(((self.d + 1) * (self.n[0] + self.n[1]), self.d), order="F")
        lib().dpgo_group_get_Xk(self.group._h, self.local, _dp(X), X.shape[0])
        return X

    def Xak(self):
        X = np.zeros(((self.d + 1) * self.n[0], self.d), order="F")
        lib().dpgo_group_get_Xak(self.group._h, self.local, _dp(X), X.shape[0])
        return X


class DistPGO:
    """Single-process dist_pgo driver loop (C++/examples/dist_pgo.cpp:446-531): every node of the graph
    hosted by one GPU.  bench.py holds the multi-process (one rank per GPU) variant."""

    def __init__(self, graph, options, X0=None, device=0):
        self.graph, self.options = graph, options
        self.group = NodeGroup(graph, range(graph.num_nodes), options, device)
        self.X0 = graph.chordal_initialization() if X0 is None else np.asfortranarray(X0)
        if self.group.initialize_global(self.X0) != 0:
            raise RuntimeError("initialize failed")
        self.group.update()

    def step(self):
        return self.group.step()

    def X(self):
        X = np.zeros(((self.graph.d + 1) * self.graph.num_poses, self.graph.d), order="F")
        self.group.scatter_global(X)
        return X

    def sum_fobj(self):
        """sum_a fobj^a == F(X_k) (invariant 1)."""
        return sum(self.group.results(k).fobj for k in range(len(self.group)))

    def evaluate(self):
        """(2F, 2|grad F|) as printed by the reference driver (dist_pgo.cpp:477-481, 523-527), from the
        per-node device reductions: F = sum_a fobj^a and |grad F|^2 = sum_a gradFnorm_a^2 (the rows of
        the global Riemannian gradient that belong to node a are exactly Proj(Dfobj^a), SURVEY Appendix
        B-1/B-4; DPGOStar::evaluate_f / evaluate_grad, DPGOStar.cpp:713-829)."""
        r = [self.group.results(k) for k in range(len(self.group))]
        return 2.0 * sum(x.fobj for x in r), 2.0 * float(np.sqrt(sum(x.gradFnorm ** 2 for x in r)))


class DPGOStar:
    """AMM-PGO* with the method names of the reference's DPGOStar
    (C++/DPGO/include/DPGO/DPGOStar.h:13-61): initialize / update / iterate / communicate.
    The master's global objective is the sum of per-node device reductions.  By default all nodes are hosted
    by one GPU; with `nodes` (this process's share) and an initialised torch.distributed process group the
    nodes are spread over one process per GPU: boundary poses travel by all-gather (after every iterate, and
    for every trial point the master evaluates), the global scalars by all-reduce."""

    def __init__(self, graph, options, device=0, nodes=None):
        self.graph, self.options = graph, options
        self.group = NodeGroup(graph, range(graph.num_nodes) if nodes is None else nodes, options, device)
        self._dist = None
        if nodes is not None and len(list(nodes)) != graph.num_nodes:
            self._connect()

    def _connect(self):
        self._dist = self.group.connect_torch()

    def initialize(self, X):
        X, ld = _fcol(X)
        return lib().dpgo_group_star_initialize(self.group._h, _dp(X), ld)

    def update(self):
        return lib().dpgo_group_star_update(self.group._h)

    def iterate(self):
        return lib().dpgo_group_star_iterate(self.group._h)

    def communicate(self):
        rc = self.group.communicate_local()
        if self._dist is not None:                   # DPGOHash::communicate across processes
            _, torch, send, gathered, ext, allgather = self._dist
            with torch.cuda.stream(ext):
                self.group.pack_sent(send.data_ptr())
            allgather()
            with torch.cuda.stream(ext):
                self.group.unpack_recv(gathered.data_ptr())
        return rc

    def state(self):
        F, f, fh, b = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        lib().dpgo_group_star_state(self.group._h, C.byref(F), C.byref(f), C.byref(fh), C.byref(b))
        return dict(F=F.value, fobj=f.value, fobjh=fh.value, branches=b.value)

    def step(self):
        return self.update() | self.iterate() | self.communicate()

    def X(self):
        X = np.zeros(((self.graph.d + 1) * self.graph.num_poses, self.graph.d), order="F")
        self.group.scatter_global(X)
        return X


CERT_UNDECIDED, CERT_NONNEGATIVE, CERT_NEGATIVE, CERT_PROVEN = 0, 1, 2, 3   # PROVEN: NodeGroup.verify only
CERT_NAMES = {0: "UNDECIDED", 1: "NONNEGATIVE", 2: "NEGATIVE", 3: "PROVEN"}
CERT_FACTOR_NOT_PD, CERT_FACTOR_PD, CERT_FACTOR_SKIPPED = 0, 1, 2
CERT_FACTOR_NAMES = {0: "NOT_PD", 1: "PD", 2: "SKIPPED"}


COV_OK, COV_NOT_PD, COV_SKIPPED = 0, 1, 2
COV_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}


class CovResult(C.Structure):
    """dpgo_cov_result_t: the outcome of NodeGroup.covariance and the sizes of its factorisation."""
    _fields_ = [("outcome", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("device_bytes", C.c_longlong), ("pivot_min", C.c_double), ("pivot_max", C.c_double),
                ("stationarity", C.c_double), ("symbolic_s", C.c_double), ("numeric_ms", C.c_double),
                ("factor_ms", C.c_double), ("selinv_ms", C.c_double), ("selinv_flops", C.c_double)]


PAIRS_OK, PAIRS_NOT_PD, PAIRS_SKIPPED = 0, 1, 2
PAIRS_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}


class PairsResult(C.Structure):
    """dpgo_pairs_result_t: the outcome of NodeGroup.pair_covariance, the sizes of its factorisation, the unit columns it
    solved, in how many batches, and the host milliseconds of its three phases."""
    _fields_ = [("outcome", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("columns", C.c_int), ("batches", C.c_int), ("reserved", C.c_int), ("device_bytes", C.c_longlong),
                ("pivot_min", C.c_double), ("pivot_max", C.c_double), ("stationarity", C.c_double), ("symbolic_s", C.c_double),
                ("factor_ms", C.c_double), ("solve_ms", C.c_double), ("gate_ms", C.c_double), ("solve_flops", C.c_double),
                ("factor_bytes", C.c_double)]


MARG_OK, MARG_NOT_PD, MARG_SKIPPED = 0, 1, 2
MARG_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}


class MargResult(C.Structure):
    """dpgo_marg_result_t: the outcome of NodeGroup.joint_marginal, the sizes of the factorisation of H, the order n of the
    dense problem, the unit columns solved, in how many batches, the pivots of the dense factorisation and the host
    milliseconds of the three phases."""
    _fields_ = [("outcome", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("info_not_pd", C.c_int), ("n", C.c_int), ("columns", C.c_int), ("batches", C.c_int), ("reserved", C.c_int),
                ("device_bytes", C.c_longlong), ("pivot_min", C.c_double), ("pivot_max", C.c_double),
                ("dense_pivot_min", C.c_double), ("dense_pivot_max", C.c_double), ("stationarity", C.c_double),
                ("symbolic_s", C.c_double), ("factor_ms", C.c_double), ("solve_ms", C.c_double), ("dense_ms", C.c_double)]


def marg_output(cov, info, logdet, order, result, want_info):
    return {"cov": cov, "info": info if want_info else None, "logdet": float(logdet[0]) if want_info else None, "order": order,
            "result": result}


def marg_plan_debug(dof, anchor, keep):
    """The column plan of a joint_marginal call (test hook, dpgo_debug_marg_plan; no device): a dict with poses (the kept poses
    other than the anchor, in LIST order), col ((K,): the first column of every kept pose, -1 for the anchor), columns,
    batches, kb."""
    K = np.ascontiguousarray(np.asarray(keep).reshape(-1), np.int32)
    poses, col, sizes = np.zeros(max(len(K), 1), np.int32), np.zeros(max(len(K), 1), np.int32), np.zeros(4, np.int32)
    if lib().dpgo_debug_marg_plan(int(dof), int(anchor), _ip(K) if len(K) else None, len(K), _ip(poses), _ip(col), _ip(sizes)) != 0:
        raise RuntimeError("dpgo_debug_marg_plan failed")
    return {"poses": poses[:sizes[0]].copy(), "col": col[:len(K)].copy(), "columns": int(sizes[1]), "batches": int(sizes[2]),
            "kb": int(sizes[3])}


def marg_rel_debug(d, X, sigma, base_pos, device=None):
    """The relative form's arithmetic on GIVEN arrays (test hooks): X (K, (d + 1) d) the kept poses' records (t, then R^T
    row-major), sigma (dof K, dof K) their joint covariance in list order, base_pos the base's position in the list.  device
    None: marg_math.h on the host (dpgo_debug_marg_rel_host; no GPU); an int: k_marg_rel alone on that HIP device
    (dpgo_debug_marg_rel).  Returns cov (dof (K - 1), dof (K - 1))."""
    dof = _dof(d)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, (d + 1) * d)
    K = X.shape[0]
    sigma = np.ascontiguousarray(sigma, np.float64)
    if d not in (2, 3) or K < 2 or sigma.shape != (dof * K, dof * K) or not 0 <= int(base_pos) < K:
        raise ValueError("marg_rel_debug: bad sizes")
    cov = np.zeros((dof * (K - 1), dof * (K - 1)))
    if device is None:
        rc = lib().dpgo_debug_marg_rel_host(int(d), K, int(base_pos), _dp(X), _dp(sigma), _dp(cov))
    else:
        rc = lib().dpgo_debug_marg_rel(int(device), int(d), K, int(base_pos), _dp(X), _dp(sigma), _dp(cov))
    if rc != 0:
        raise RuntimeError("dpgo_debug_marg_rel failed")
    return cov


def marg_dense_debug(A, device=0):
    """The dense tail of joint_marginal on a GIVEN symmetric matrix (test hook, dpgo_debug_marg_dense): the gather in batches of
    64 columns, the one-front factorisation, its inverse and the log-determinant.  Returns a dict: cov (the gathered copy of
    A), info (A^-1), logdet (log det A), result (MargResult; info_not_pd: info and logdet are zeros)."""
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    if A.ndim != 2 or A.shape != (n, n) or n < 1:
        raise ValueError("marg_dense_debug: A is not square")
    cov, info, logdet, r = np.zeros((n, n)), np.zeros((n, n)), np.zeros(1), MargResult()
    if lib().dpgo_debug_marg_dense(int(device), n, _dp(A), _dp(cov), _dp(info), _dp(logdet), C.byref(r)) != 0:
        raise RuntimeError("dpgo_debug_marg_dense failed")
    return {"cov": cov, "info": info, "logdet": float(logdet[0]), "result": r}


CAND_OK, CAND_NOT_PD, CAND_SKIPPED = 0, 1, 2
CAND_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}


class CandResult(C.Structure):
    """dpgo_cand_result_t: the outcome of NodeGroup.candidate_set, the sizes of the factorisation of H, the order n = dof m of the
    joint problem, the distinct end poses, the unit columns solved and in how many batches, how many candidates were chosen,
    the pivots of the dense factorisation of S and the host milliseconds of the four phases."""
    _fields_ = [("outcome", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("joint_not_pd", C.c_int), ("n", C.c_int), ("poses", C.c_int), ("columns", C.c_int), ("batches", C.c_int),
                ("n_selected", C.c_int), ("reserved", C.c_int), ("device_bytes", C.c_longlong), ("pivot_min", C.c_double),
                ("pivot_max", C.c_double), ("dense_pivot_min", C.c_double), ("dense_pivot_max", C.c_double),
                ("stationarity", C.c_double), ("symbolic_s", C.c_double), ("factor_ms", C.c_double), ("solve_ms", C.c_double),
                ("dense_ms", C.c_double), ("select_ms", C.c_double)]


def cand_output(a, r, want_joint):
    k = r.n_selected
    sc = a["scalars"]
    return {"cov": a["cov"], "S": a["S"], "residual": a["residual"], "info": a["info"] if want_joint else None,
            "logdet": float(sc[0]) if want_joint else None, "d2_joint": float(sc[1]) if want_joint else None,
            "gain_all": float(sc[2]) if want_joint else None, "selected": a["selected"][:k].copy(), "steps": a["steps"][:k].copy(),
            "gain_selected": float(sc[3]), "d2_selected": float(sc[4]), "poses": a["poses"][:r.poses].copy(), "result": r}


def cand_innov_debug(d, X, sigma, kpos, candidates, device=None):
    """The block arithmetic of candidate_set on GIVEN arrays (test hooks): X (K, (d + 1) d) the records of the listed poses (t,
    then R^T row-major), sigma (dof K, dof K) their joint covariance in list order, kpos (m, 2) the positions of every
    candidate's ends in the list, candidates as candidate_set's.  device None: cand_math.h on the host
    (dpgo_debug_cand_innov_host; no GPU); an int: k_cand_innov and k_cand_resid alone on that HIP device.  Returns a dict: cov,
    S (dof m, dof m), residual (dof m,)."""
    dof = _dof(d)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, (d + 1) * d)
    K = X.shape[0]
    sigma = np.ascontiguousarray(sigma, np.float64)
    kp = np.ascontiguousarray(np.asarray(kpos).reshape(-1, 2), np.int32)
    m = len(kp)
    if d not in (2, 3) or m < 1 or K < 2 or sigma.shape != (dof * K, dof * K) or kp.min() < 0 or kp.max() >= K:
        raise ValueError("cand_innov_debug: bad sizes")
    cand = _cand_pack(d, m, candidates)
    n = dof * m
    cov, S, r = np.zeros((n, n)), np.zeros((n, n)), np.zeros(n)
    if device is None:
        rc = lib().dpgo_debug_cand_innov_host(int(d), m, K, _ip(kp), _dp(X), _dp(sigma), _dp(cand), _dp(cov), _dp(S), _dp(r))
    else:
        rc = lib().dpgo_debug_cand_innov(int(device), int(d), m, K, _ip(kp), _dp(X), _dp(sigma), _dp(cand), _dp(cov), _dp(S), _dp(r))
    if rc != 0:
        raise RuntimeError("dpgo_debug_cand_innov failed")
    return {"cov": cov, "S": S, "residual": r}


def cand_select_debug(d, S, r, weights, budget, d2_max=0.0, device=None, selected=None, steps=None):
    """The selection of candidate_set on a GIVEN S (dof m, dof m), r (dof m,) and weights (m, 2: kappa, tau), no graph (test hooks).
    device None: the same steps on the host (dpgo_debug_cand_select_host; no GPU); an int: k_cand_score / k_cand_update on that
    HIP device.  selected (budget,) and steps (budget, 4) start as given (default -1 and zeros): only the chosen steps are
    written, entries from n_selected on keep their values.  Returns a dict: selected, steps (whole arrays), n_selected,
    gain_selected, d2_selected."""
    dof = _dof(d)
    S = np.ascontiguousarray(S, np.float64)
    r = np.ascontiguousarray(r, np.float64).reshape(-1)
    w = np.ascontiguousarray(weights, np.float64).reshape(-1, 2)
    m, budget = len(w), int(budget)
    if d not in (2, 3) or m < 1 or budget < 0 or S.shape != (dof * m, dof * m) or r.shape != (dof * m,):
        raise ValueError("cand_select_debug: bad sizes")
    sel = np.full(max(budget, 1), -1, np.int32) if selected is None else np.ascontiguousarray(selected, np.int32).copy()
    stp = np.zeros((max(budget, 1), 4)) if steps is None else np.ascontiguousarray(steps, np.float64).copy()
    if len(sel) < max(budget, 1) or stp.shape != (len(sel), 4):
        raise ValueError("cand_select_debug: selected / steps are shorter than the budget")
    sums, nsel = np.zeros(2), np.zeros(1, np.int32)
    if device is None:
        rc = lib().dpgo_debug_cand_select_host(int(d), m, budget, float(d2_max), _dp(S), _dp(r), _dp(w), _ip(sel), _dp(stp), _dp(sums),
                                               _ip(nsel))
    else:
        rc = lib().dpgo_debug_cand_select(int(device), int(d), m, budget, float(d2_max), _dp(S), _dp(r), _dp(w), _ip(sel), _dp(stp),
                                          _dp(sums), _ip(nsel))
    if rc != 0:
        raise RuntimeError("dpgo_debug_cand_select failed (a weight that is not positive, or bad sizes)")
    return {"selected": sel[:budget], "steps": stp[:budget], "n_selected": int(nsel[0]), "gain_selected": float(sums[0]),
            "d2_selected": float(sums[1])}


def pack_candidates(d, npairs, R, t, kappa, tau):
    """(npairs, d^2 + d + 2): R row-major, t, kappa, tau per candidate, as dpgo_group_pair_covariance reads them."""
    out = np.zeros((npairs, d * d + d + 2))
    out[:, :d * d] = np.asarray(R, np.float64).reshape(npairs, d * d)
    out[:, d * d:d * d + d] = np.asarray(t, np.float64).reshape(npairs, d)
    out[:, d * d + d] = np.asarray(kappa, np.float64).reshape(npairs)
    out[:, d * d + d + 1] = np.asarray(tau, np.float64).reshape(npairs)
    return out


def pairs_output(joint, rel, gate, result, gated, threshold):
    out = {"joint": joint, "rel": rel, "result": result}
    if gated:
        out.update(d2=gate[:, 0].copy(), not_pd=gate[:, 1] != 0, residual=gate[:, 2:].copy())
        if threshold is not None:
            out["accept"] = (~out["not_pd"]) & (out["d2"] <= float(threshold)) & (result.outcome == PAIRS_OK)
    return out


def pairs_plan_debug(dof, anchor, pairs):
    """The column plan of a pair_covariance call (test hook, dpgo_debug_pairs_plan; no device): a dict with poses (the distinct
    non-anchor poses, ascending), pair_col ((npairs, 2): the first column of p and q, -1 for the anchor), columns, batches,
    kb."""
    P = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)
    poses, cols, sizes = np.zeros(max(2 * len(P), 1), np.int32), np.zeros((max(len(P), 1), 2), np.int32), np.zeros(4, np.int32)
    if lib().dpgo_debug_pairs_plan(int(dof), int(anchor), _ip(P) if len(P) else None, len(P), _ip(poses), _ip(cols), _ip(sizes)) != 0:
        raise RuntimeError("dpgo_debug_pairs_plan failed")
    return {"poses": poses[:sizes[0]].copy(), "pair_col": cols[:len(P)].copy(), "columns": int(sizes[1]), "batches": int(sizes[2]),
            "kb": int(sizes[3])}


def pairs_gate_debug(d, recp, recq, joint, candidate=None):
    """The arithmetic of one pair on the host (test hook, dpgo_debug_pairs_gate; no device), the code the device runs per
    pair.  recp / recq: the pose records ((d + 1) x d: t, then R^T); joint (3, dof, dof); candidate: None or (R, t, kappa,
    tau).  Returns (rel, None) or (rel, (d2, not_pd, residual))."""
    dof = _dof(d)
    recp, recq = np.ascontiguousarray(recp, np.float64), np.ascontiguousarray(recq, np.float64)
    joint = np.ascontiguousarray(joint, np.float64)
    if recp.size != (d + 1) * d or recq.size != (d + 1) * d or joint.size != 3 * dof * dof:
        raise ValueError("pairs_gate_debug: bad sizes")
    cand = None if candidate is None else pack_candidates(d, 1, *candidate)
    rel, gate = np.zeros((dof, dof)), np.zeros(2 + dof)
    if lib().dpgo_debug_pairs_gate(int(d), _dp(recp), _dp(recq), _dp(joint), None if cand is None else _dp(cand), _dp(rel), _dp(gate)) != 0:
        raise RuntimeError("dpgo_debug_pairs_gate failed (d, or a candidate weight that is not positive)")
    return rel, (None if cand is None else (float(gate[0]), bool(gate[1]), gate[2:].copy()))


SENS_OK, SENS_NOT_PD, SENS_SKIPPED = 0, 1, 2
SENS_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}


class SensResult(C.Structure):
    """dpgo_sens_result_t: the outcome of NodeGroup.sensitivity, the sizes of its factorisation, the columns it solved, in how
    many batches, for how many edges, and the host milliseconds of its three phases."""
    _fields_ = [("outcome", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("columns", C.c_int), ("batches", C.c_int), ("edges", C.c_int), ("device_bytes", C.c_longlong),
                ("pivot_min", C.c_double), ("pivot_max", C.c_double), ("stationarity", C.c_double), ("symbolic_s", C.c_double),
                ("factor_ms", C.c_double), ("solve_ms", C.c_double), ("edge_ms", C.c_double)]


RELY_OK, RELY_NOT_PD, RELY_SKIPPED = 0, 1, 2
RELY_AUTO, RELY_SELINV, RELY_SOLVE = 0, 1, 2
RELY_NAMES = {0: "OK", 1: "NOT_PD", 2: "SKIPPED"}
RELY_METHOD_NAMES = {0: "AUTO", 1: "SELINV", 2: "SOLVE"}


class RelyResult(C.Structure):
    """dpgo_rely_result_t: the outcome of NodeGroup.edge_reliability, the method it ran, the sizes of its factorisation, how many
    edges were listed, flagged (C not positive definite) and unweighted, the sum of the redundancies in list order, the bytes
    either method would allocate, and the host milliseconds of its three phases."""
    _fields_ = [("outcome", C.c_int), ("method_used", C.c_int), ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int),
                ("max_front", C.c_int), ("edges", C.c_int), ("flagged", C.c_int), ("unweighted", C.c_int), ("columns", C.c_int),
                ("batches", C.c_int), ("reserved", C.c_int), ("device_bytes", C.c_longlong), ("device_bytes_selinv", C.c_longlong),
                ("device_bytes_solve", C.c_longlong), ("redundancy_sum", C.c_double), ("pivot_min", C.c_double),
                ("pivot_max", C.c_double), ("stationarity", C.c_double), ("symbolic_s", C.c_double), ("factor_ms", C.c_double),
                ("inverse_ms", C.c_double), ("edge_ms", C.c_double)]


def _rely_arg(graph, edges):
    """The arrays of an edge_reliability call: (records, rel, joint, (edges pointer or None, count))."""
    dof = _dof(graph.d)
    if edges is None:
        n, args = graph.num_edges, (None, 0)
    else:
        E = np.ascontiguousarray(np.asarray(edges).reshape(-1), np.int32)
        n, args = len(E), (_ip(E), len(E))   # (the pointer keeps E alive)
    return np.zeros((n, 6 + 2 * dof)), np.zeros((n, dof, dof)), np.zeros((n, 3, dof, dof)), args


def rely_output(d, records, rel, joint, result):
    dof = _dof(d)
    return dict(records=records, d2_loo=records[:, 0], flag=records[:, 1].astype(np.int64), redundancy=records[:, 2],
                redundancy_trans=records[:, 3], d2_own=records[:, 4], influence=records[:, 5], residual=records[:, 6:6 + dof],
                r_loo=records[:, 6 + dof:], rel=rel, joint=joint, result=result)


def rely_edge_debug(d, rel, r, kappa, tau, device=None):
    """The record arithmetic of NodeGroup.edge_reliability on given arrays (test hooks): rel (n, dof, dof), r (n, dof), kappa, tau
    (n).  device None: on the host (dpgo_debug_rely_edge_host; no GPU); an int: k_rely_edge alone on that HIP device
    (dpgo_debug_rely_edge).  Returns records (n, 6 + 2 dof)."""
    dof = _dof(d)
    rel = np.ascontiguousarray(rel, np.float64).reshape(-1, dof, dof)
    n = rel.shape[0]
    r = np.ascontiguousarray(r, np.float64).reshape(-1, dof)
    kappa, tau = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,))) for v in (kappa, tau))
    if d not in (2, 3) or r.shape[0] != n:
        raise ValueError("rely_edge_debug: bad sizes")
    rec = np.zeros((n, 6 + 2 * dof))
    if device is None:
        rc = lib().dpgo_debug_rely_edge_host(int(d), n, _dp(rel), _dp(r), _dp(kappa), _dp(tau), _dp(rec))
    else:
        rc = lib().dpgo_debug_rely_edge(int(device), int(d), n, _dp(rel), _dp(r), _dp(kappa), _dp(tau), _dp(rec))
    if rc != 0:
        raise RuntimeError("dpgo_debug_rely_edge failed")
    return rec


def ml_rely_edge_debug(d, J, joint, omega, r, sign=-1, device=None):
    """The arithmetic of NodeGroup.ml_edge_reliability (sign -1) and ml_pair_gate (sign +1) on given arrays (test hooks): J
    (n, 2, dof, dof) = [J_p | J_q], joint (n, 3, dof, dof), omega (n, dof, dof), r (n, dof).  device None: on the host
    (dpgo_debug_ml_rely_edge_host; no GPU); an int: k_ml_rel and k_ml_rely_edge alone on that HIP device
    (dpgo_debug_ml_rely_edge).  Returns (rel (n, dof, dof), records (n, 6 + 2 dof) or (n, 2 + dof))."""
    dof = _dof(d)
    J = np.ascontiguousarray(J, np.float64).reshape(-1, 2, dof, dof)
    n = J.shape[0]
    joint = np.ascontiguousarray(joint, np.float64).reshape(-1, 3, dof, dof)
    omega = np.ascontiguousarray(omega, np.float64).reshape(-1, dof, dof)
    r = np.ascontiguousarray(r, np.float64).reshape(-1, dof)
    if d not in (2, 3) or joint.shape[0] != n or omega.shape[0] != n or r.shape[0] != n:
        raise ValueError("ml_rely_edge_debug: bad sizes")
    rel, rec = np.zeros((n, dof, dof)), np.zeros((n, 6 + 2 * dof if sign < 0 else 2 + dof))
    if device is None:
        rc = lib().dpgo_debug_ml_rely_edge_host(int(d), n, int(sign), _dp(J), _dp(joint), _dp(omega), _dp(r), _dp(rel), _dp(rec))
    else:
        rc = lib().dpgo_debug_ml_rely_edge(int(device), int(d), n, int(sign), _dp(J), _dp(joint), _dp(omega), _dp(r), _dp(rel),
                                           _dp(rec))
    if rc != 0:
        raise RuntimeError("dpgo_debug_ml_rely_edge failed (bad sizes, a sign that is not +-1, or an omega that is not positive definite)")
    return rel, rec


def sens_edge_debug(graph, X, lam):
    """Debug, no GPU: the per-edge arithmetic of the sensitivities' kernel on the host (dpgo_debug_sens_edge_host) for one
    adjoint `lam` (dof N by global pose, used as given).  Returns (sens, phi): (num_edges, 2 + dof) in NodeGroup.sensitivity's
    order, and phi_e = lam_i' ghat_e(i) + lam_j' ghat_e(j) per edge."""
    X, ld = _fcol(X)
    dof, m = _dof(graph.d), graph.num_edges
    lam = np.ascontiguousarray(lam, np.float64)
    if lam.shape != (dof * graph.num_poses,):
        raise ValueError("sens_edge_debug: lam must have dof N entries")
    sens, phi = np.zeros((m, 2 + dof)), np.zeros(m)
    if lib().dpgo_debug_sens_edge_host(graph._h, _dp(X), ld, _dp(lam), _dp(sens), _dp(phi)) != 0:
        raise ValueError("dpgo_debug_sens_edge_host failed (a short X, or an edge outside the graph)")
    return sens, phi


def _hat_generators(d):
    if d == 2:
        return [np.array([[0.0, -1.0], [1.0, 0.0]])]
    return [np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0.0, 0, 1], [0, 0, 0], [-1, 0, 0]]),
            np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 0]])]


def tangent_gradient(X, G):
    """The tangent gradient (dof N, by global pose, `covariance`'s coordinates) of a scalar whose ambient gradient at X is G,
    an array shaped like X ((d+1)N x d: row p the derivative in t_p, rows N + d p ... in the rows of Y_p = R_p^T):
    c_p[a < d] = G_t[p, a], c_p[d + k] = <G_R, R_p hat(e_k)> = <G_Y, -hat(e_k) Y_p>.  What NodeGroup.sensitivity takes as
    a column of `upstream`."""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    d = X.shape[1]
    if G.shape != X.shape or X.shape[0] % (d + 1):
        raise ValueError("tangent_gradient: G must be shaped like X, (d+1)N x d")
    N, dof = X.shape[0] // (d + 1), _dof(d)
    Y, GY = X[N:].reshape(N, d, d), G[N:].reshape(N, d, d)
    c = np.zeros((N, dof))
    c[:, :d] = G[:N]
    for k, E in enumerate(_hat_generators(d)):
        c[:, d + k] = -np.einsum("rq,pqc,prc->p", E, Y, GY)
    return c.reshape(-1)


def unit_upstream(N, d, pose):
    """(dof N, dof): the dof unit columns of one pose -- NodeGroup.sensitivity with them gives the influence of every
    measurement on each tangent coordinate of that pose."""
    dof = _dof(d)
    if not 0 <= pose < N:
        raise ValueError("unit_upstream: the pose is not in the graph")
    U_ = np.zeros((dof * N, dof), order="F")
    U_[dof * pose:dof * pose + dof] = np.eye(dof)
    return U_


POLISH_CONVERGED, POLISH_MAX_STEPS, POLISH_STALLED, POLISH_SKIPPED = 0, 1, 2, 3
POLISH_NAMES = {0: "CONVERGED", 1: "MAX_STEPS", 2: "STALLED", 3: "SKIPPED"}


class PolishOptions(C.Structure):
    """dpgo_polish_options_t: max_steps, max_tries, rel_tol, grad_tol, anchor."""
    _fields_ = [("max_steps", C.c_int), ("max_tries", C.c_int), ("rel_tol", C.c_double), ("grad_tol", C.c_double),
                ("anchor", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_polish_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("PolishOptions has no field %r" % k)
            setattr(self, k, v)


class PolishResult(C.Structure):
    """dpgo_polish_result_t: the outcome of NodeGroup.polish, its counts, F and |g| at both ends, the sizes of its factorisation
    and its times."""
    _fields_ = [("outcome", C.c_int), ("steps", C.c_int), ("factorisations", C.c_int), ("indefinite", C.c_int),
                ("F_initial", C.c_double), ("F_final", C.c_double), ("grad_initial", C.c_double), ("grad_final", C.c_double),
                ("hmax", C.c_double), ("mu_final", C.c_double), ("pivot_min", C.c_double), ("pivot_max", C.c_double),
                ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("device_bytes", C.c_longlong), ("symbolic_s", C.c_double), ("total_ms", C.c_double), ("factor_ms", C.c_double),
                ("solve_ms", C.c_double), ("other_ms", C.c_double)]


class MlResult(C.Structure):
    """dpgo_ml_result_t: `polish` (a PolishResult, whose fields read through), near_pi at the final point, and
    chi2_initial / chi2_final = 2 F_ml at both ends."""
    _fields_ = [("polish", PolishResult), ("near_pi", C.c_longlong), ("chi2_initial", C.c_double), ("chi2_final", C.c_double)]

    def __getattr__(self, name):   # (only reached where the struct itself has no such field)
        if name != "polish" and name in dict(PolishResult._fields_):
            return getattr(self.polish, name)
        raise AttributeError(name)


MODES_CONVERGED, MODES_MAX_ITERS, MODES_STALLED, MODES_SKIPPED = 0, 1, 2, 3
MODES_NAMES = {0: "CONVERGED", 1: "MAX_ITERS", 2: "STALLED", 3: "SKIPPED"}


class ModesOptions(C.Structure):
    """dpgo_modes_options_t: guard, max_iters, max_tries, want_escape, rel_tol, shift, seed."""
    _fields_ = [("guard", C.c_int), ("max_iters", C.c_int), ("max_tries", C.c_int), ("want_escape", C.c_int),
                ("rel_tol", C.c_double), ("shift", C.c_double), ("seed", C.c_ulonglong)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_modes_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("ModesOptions has no field %r" % k)
            setattr(self, k, v)


class ModesResult(C.Structure):
    """dpgo_modes_result_t: the outcome of NodeGroup.hessian_modes, its counts, the shift, F at X and at the escape point, the
    sizes of the factorisation and the host milliseconds of the phases."""
    _fields_ = [("outcome", C.c_int), ("iterations", C.c_int), ("factorisations", C.c_int), ("shift_tries", C.c_int),
                ("block", C.c_int), ("negative", C.c_int), ("escaped", C.c_int), ("reserved", C.c_int),
                ("unknowns", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("device_bytes", C.c_longlong), ("mu", C.c_double), ("hmax", C.c_double), ("stationarity", C.c_double),
                ("escape_alpha", C.c_double), ("F", C.c_double), ("F_escape", C.c_double), ("pivot_min", C.c_double),
                ("pivot_max", C.c_double), ("symbolic_s", C.c_double), ("factor_ms", C.c_double), ("solve_ms", C.c_double),
                ("gram_ms", C.c_double), ("ritz_ms", C.c_double), ("update_ms", C.c_double), ("total_ms", C.c_double)]


def _modes_blocks(b, *arrays):
    """The (n, ld) row-major blocks of a modes_*_debug call and their shape: (n, ld, the arrays as contiguous float64)."""
    out = [np.ascontiguousarray(a, np.float64) for a in arrays]
    n, ld = out[0].shape
    if any(a.shape != (n, ld) for a in out) or ld < b or b not in (16, 32, 48, 64) or n < 1:
        raise ValueError("modes debug: blocks must be (n, ld) with ld >= b, b in {16, 32, 48, 64}")
    return n, ld, out


def modes_init_debug(V, b, seed=1, anchor_row0=-1, dof=0, device=0):
    """k_modes_init on a GIVEN array (test hook): V (n, ld) -- its columns 0 ... b are overwritten with the start block, entry
    (i, j) a pure function of (seed, i, j) in (-1, 1), zeros on the rows anchor_row0 ... anchor_row0 + dof; everything else
    keeps the caller's values.  Returns the new array."""
    n, ld, (V,) = _modes_blocks(b, V)
    V = V.copy()
    rc = lib().dpgo_debug_modes_init(int(device), n, int(b), ld, int(anchor_row0), int(dof), int(seed), _dp(V))
    if rc != 0:
        raise RuntimeError("dpgo_debug_modes_init failed (%d; -2: a write outside the array)" % rc)
    return V


def modes_gram_debug(W, V, b, device=0):
    """k_modes_gram and k_modes_reduce on GIVEN blocks W, V (n, ld) (test hook): (G, T), b x b each -- W'W and the mirrored
    lower triangle of W'V over the columns 0 ... b."""
    n, ld, (W, V) = _modes_blocks(b, W, V)
    G, T = np.zeros((b, b)), np.zeros((b, b))
    rc = lib().dpgo_debug_modes_gram(int(device), n, int(b), ld, _dp(W), _dp(V), _dp(G), _dp(T))
    if rc != 0:
        raise RuntimeError("dpgo_debug_modes_gram failed (%d; -2: a write outside the arrays)" % rc)
    return G, T


def modes_update_debug(W, V, Cm, theta, b, anchor_row0=-1, dof=0, device=0):
    """k_modes_update and k_modes_reduce on GIVEN blocks (test hook): returns (V' = W C on the columns 0 ... b with zeros on the
    anchor's rows -- the other columns keep V's values --, rr (b,), vv (b,)): the column sums of (V C - (W C) diag(theta))^2 and
    of (W C)^2."""
    n, ld, (W, V) = _modes_blocks(b, W, V)
    V = V.copy()
    Cm = np.ascontiguousarray(Cm, np.float64)
    theta = np.ascontiguousarray(theta, np.float64)
    if Cm.shape != (b, b) or theta.shape != (b,):
        raise ValueError("modes_update_debug: C must be (b, b) and theta (b,)")
    rr, vv = np.zeros(b), np.zeros(b)
    rc = lib().dpgo_debug_modes_update(int(device), n, int(b), ld, int(anchor_row0), int(dof), _dp(W), _dp(V), _dp(Cm), _dp(theta),
                                       _dp(rr), _dp(vv))
    if rc != 0:
        raise RuntimeError("dpgo_debug_modes_update failed (%d; -2: a write outside the arrays)" % rc)
    return V, rr, vv


def modes_ritz_debug(G=None, T=None, W=None, V=None, b=None, device=0):
    """The host's eigenproblem of hessian_modes (test hook).  With G, T (b, b; the lower triangles are read): modes_ritz alone, no
    GPU (dpgo_debug_modes_ritz_host).  With W, V (n, ld) and b: the Gram matrices on the device first.  Returns (theta (used,)
    ascending, C (b, b) with C'GC = I on the first `used` columns and e_j / sqrt(G_jj) on the others, used)."""
    used = C.c_int(0)
    if G is not None:
        G = np.ascontiguousarray(G, np.float64)
        T = np.ascontiguousarray(T, np.float64)
        b = G.shape[0]
        if G.shape != (b, b) or T.shape != (b, b):
            raise ValueError("modes_ritz_debug: G and T must be (b, b)")
        theta, Cm = np.zeros(b), np.zeros((b, b))
        rc = lib().dpgo_debug_modes_ritz_host(b, _dp(G), _dp(T), _dp(theta), _dp(Cm), C.byref(used))
    else:
        n, ld, (W, V) = _modes_blocks(b, W, V)
        theta, Cm = np.zeros(b), np.zeros((b, b))
        rc = lib().dpgo_debug_modes_ritz(int(device), n, int(b), ld, _dp(W), _dp(V), _dp(theta), _dp(Cm), C.byref(used))
    if rc != 0:
        raise RuntimeError("dpgo_debug_modes_ritz failed (%d: bad sizes, or not one column of G has a positive diagonal entry)" % rc)
    return theta[:used.value].copy(), Cm, used.value


GNC_TLS, GNC_GM = 0, 1
GNC_CONVERGED, GNC_ALL_INLIERS, GNC_MAX_LEVELS, GNC_INNER_FAILED, GNC_SKIPPED = 0, 1, 2, 3, 4
GNC_NAMES = {0: "CONVERGED", 1: "ALL_INLIERS", 2: "MAX_LEVELS", 3: "INNER_FAILED", 4: "SKIPPED"}


class GncOptions(C.Structure):
    """dpgo_gnc_options_t: kind (GNC_TLS, GNC_GM), barc2, mu_step, max_levels, and inner, the PolishOptions of every inner
    solve (its anchor included).  Keywords that are fields of PolishOptions go to inner."""
    _fields_ = [("kind", C.c_int), ("barc2", C.c_double), ("mu_step", C.c_double), ("max_levels", C.c_int), ("inner", PolishOptions)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_gnc_options_default(C.byref(self))
        for k, v in kw.items():
            if k in dict(PolishOptions._fields_):
                setattr(self.inner, k, v)
            elif k in dict(self._fields_) and k != "inner":
                setattr(self, k, v)
            else:
                raise TypeError("GncOptions has no field %r" % k)


class GncResult(C.Structure):
    """dpgo_gnc_result_t: the outcome of NodeGroup.gnc, its levels and inner counts, mu at both ends, F at unit weights at the
    start and F_w, F_mu at the end, the counts of the final weights over the robust set, the bytes and the times."""
    _fields_ = [("outcome", C.c_int), ("levels", C.c_int), ("steps", C.c_int), ("factorisations", C.c_int), ("inner_outcome", C.c_int),
                ("mu_initial", C.c_double), ("mu_final", C.c_double), ("s_max_initial", C.c_double), ("F_initial", C.c_double),
                ("F_weighted_final", C.c_double), ("F_surrogate_final", C.c_double), ("num_robust", C.c_int), ("num_zero", C.c_int),
                ("num_one", C.c_int), ("num_between", C.c_int), ("num_outliers", C.c_int), ("device_bytes", C.c_longlong),
                ("symbolic_s", C.c_double), ("total_ms", C.c_double), ("edge_ms", C.c_double), ("inner_ms", C.c_double)]


class MlGncResult(C.Structure):
    """dpgo_ml_gnc_result_t: `gnc` (a GncResult, whose fields read through) on chi2 -- s_max_initial = max_R chi2 at X0,
    num_outliers the edges of R with chi2 > barc2 at the final point -- then near_pi, the edges with w > 0 within 1e-3 of pi at
    the final point, and near_pi_all, every such edge."""
    _fields_ = [("gnc", GncResult), ("near_pi", C.c_longlong), ("near_pi_all", C.c_longlong)]

    def __getattr__(self, name):   # (only reached where the struct itself has no such field)
        if name != "gnc" and name in dict(GncResult._fields_):
            return getattr(self.gnc, name)
        raise AttributeError(name)


def gnc_weight_debug(kind, mu, barc2, s):
    """Debug, no GPU: (w, rho) of graduated non-convexity's surrogate at the values s >= 0, through the kernel's own arithmetic
    (dpgo_debug_gnc_weight_host)."""
    s = np.ascontiguousarray(s, np.float64).ravel()
    w, rho = np.zeros(len(s)), np.zeros(len(s))
    if lib().dpgo_debug_gnc_weight_host(int(kind), float(mu), float(barc2), _dp(s), len(s), _dp(w), _dp(rho)) != 0:
        raise ValueError("dpgo_debug_gnc_weight_host failed (a kind outside {0, 1}, mu or barc2 not finite and positive, a negative s)")
    return w, rho


STAIR_SOLVED, STAIR_MAX_RANK, STAIR_SADDLE, STAIR_SKIPPED = 0, 1, 2, 3
STAIR_NAMES = {0: "SOLVED", 1: "MAX_RANK", 2: "SADDLE", 3: "SKIPPED"}


class StaircaseOptions(C.Structure):
    """dpgo_staircase_options_t: the optimiser's options under SESyncOpts' names, r_max (0: 2d), precondition, polish,
    min_eig_num_tol, max_factor_bytes."""
    _fields_ = [("grad_norm_tol", C.c_double), ("preconditioned_grad_norm_tol", C.c_double), ("rel_func_decrease_tol", C.c_double),
                ("stepsize_tol", C.c_double), ("max_iterations", C.c_int), ("max_tCG_iterations", C.c_int),
                ("STPCG_kappa", C.c_double), ("STPCG_theta", C.c_double), ("r_max", C.c_int), ("precondition", C.c_int),
                ("polish", C.c_int), ("reserved", C.c_int), ("min_eig_num_tol", C.c_double), ("max_factor_bytes", C.c_longlong)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_staircase_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("StaircaseOptions has no field %r" % k)
            setattr(self, k, v)


class StaircaseResult(C.Structure):
    """dpgo_staircase_result_t: the outcome of NodeGroup.staircase, the last certificate, the ranks, the counts, F at the four
    points, gap, the singular values, the bytes and the times."""
    _fields_ = [("outcome", C.c_int), ("cert_status", C.c_int), ("final_rank", C.c_int), ("levels", C.c_int),
                ("tnt_iterations", C.c_int), ("hess_products", C.c_int), ("replaced_by_input", C.c_int), ("polish_outcome", C.c_int),
                ("theta", C.c_double), ("stationarity", C.c_double), ("F_initial", C.c_double), ("F_sdp", C.c_double),
                ("F_rounded", C.c_double), ("F_final", C.c_double), ("gap", C.c_double), ("sigma", C.c_double * 6),
                ("device_bytes", C.c_longlong), ("optimise_ms", C.c_double), ("verify_ms", C.c_double), ("round_ms", C.c_double),
                ("total_ms", C.c_double)]


class CertOptions(C.Structure):
    """dpgo_cert_options_t: eta (SESync.h:88), tau (LOBPCG.h:138), max_iters, precondition, stop_on_negative, refresh_every, seed."""
    _fields_ = [("eta", C.c_double), ("tau", C.c_double), ("max_iters", C.c_int), ("precondition", C.c_int),
                ("stop_on_negative", C.c_int), ("refresh_every", C.c_int), ("seed", C.c_ulonglong)]

    def __init__(self, **kw):
        super().__init__()
        lib().dpgo_cert_options_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class CertResult(C.Structure):
    """dpgo_cert_result_t."""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("restarts", C.c_int), ("theta", C.c_double),
                ("residual", C.c_double), ("S_norm_est", C.c_double), ("stationarity", C.c_double)]


class CertFactor(C.Structure):
    """dpgo_cert_factor_t: the outcome of fast_verification STEP 1 and the sizes of its factorisation."""
    _fields_ = [("outcome", C.c_int), ("fronts", C.c_int), ("levels", C.c_int), ("max_front", C.c_int),
                ("factor_entries", C.c_longlong), ("factor_bytes", C.c_longlong), ("eta", C.c_double),
                ("pivot_min", C.c_double), ("pivot_max", C.c_double), ("stationarity", C.c_double),
                ("symbolic_s", C.c_double), ("numeric_s", C.c_double)]


def rayleigh_ritz(A, B, nblk):
    """The host's Rayleigh-Ritz step (dpgo_debug_rayleigh_ritz): A, B symmetric n x n, n = ns * nblk.  Returns (theta, C, used):
    the ns smallest Ritz values, C (n x ns) with C' B C = I and C' A C = diag(theta), and the number of blocks used (a
    mass-matrix pivot below 1e-12 after scaling drops the last block)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    n = A.shape[0]
    if A.shape != (n, n) or B.shape != (n, n) or n % nblk:
        raise ValueError("rayleigh_ritz: A and B must be square of a size divisible by nblk")
    ns = n // nblk
    theta, Cm, used = np.zeros(ns), np.zeros((n, ns)), np.zeros(1, np.int32)
    if lib().dpgo_debug_rayleigh_ritz(ns, int(nblk), _dp(A), _dp(B), _dp(theta), _dp(Cm), _ip(used)) != 0:
        raise RuntimeError("dpgo_debug_rayleigh_ritz failed")
    return theta, Cm, int(used[0])


class PCMOptions(C.Structure):
    """DPGO::PCM::Options (C++/DPGO/include/DPGO/PCM.h:13-19)."""
    _fields_ = [("tolerance", C.c_double), ("weighted", C.c_int)]


class PCM:
    """DPGO::PCM (C++/DPGO/include/DPGO/PCM.h, C++/DPGO/src/PCM.cpp:5-235): pairwise consistency of the measurements
    between two nodes, tested on the GPU (fp64), and the maximum clique of consistent ones (host).  update() takes the
    graph and the GLOBAL iterate X ((d+1)N x d) instead of the reference's measurements + index; measurements() are
    edge indices of the graph.  There is no CPU path: constructing one without a HIP device raises."""

    def __init__(self, device=0):
        h = C.c_void_p()
        if lib().dpgo_pcm_create(int(device), C.byref(h)) != 0:
            raise RuntimeError("dpgo_pcm_create failed (no HIP device?); there is no CPU path")
        self._h = h
        self.m = 0
        self.tolerance, self.weighted = 0.2, False

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dpgo_pcm_free(self._h)
            self._h = None

    def update(self, graph, alpha, beta, X, tolerance=0.2, weighted=False):
        """PCM::update: returns m, the number of alpha-beta measurements (-1 raises ValueError)."""
        X, ld = _fcol(X)
        o = PCMOptions(float(tolerance), int(bool(weighted)))
        m = lib().dpgo_pcm_update(self._h, graph._h, int(alpha), int(beta), _dp(X), ld, C.byref(o))
        if m < 0:
            self.m = 0
            raise ValueError("PCM.update(%d, %d) failed" % (alpha, beta))
        self.m, self.tolerance, self.weighted = m, float(tolerance), bool(weighted)
        return m

    def measurements(self):
        ids = np.zeros(max(self.m, 1), np.int32)
        lib().dpgo_pcm_measurements(self._h, _ip(ids))
        return ids[:self.m]

    def adjacency(self):
        """PCM::adjancecy_matrix: m x m 0/1 (uint8), symmetric, diagonal 1."""
        A = np.zeros((self.m, self.m), np.uint8)
        if self.m and lib().dpgo_pcm_adjacency(self._h, A.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("dpgo_pcm_adjacency failed")
        return A

    def errors(self):
        """Debug: the m x m pair errors (m <= 4096)."""
        E = np.zeros((self.m, self.m))
        if self.m and lib().dpgo_pcm_errors(self._h, _dp(E)) != 0:
            raise RuntimeError("dpgo_pcm_errors failed (m = %d > 4096?)" % self.m)
        return E

    def _solve(self, exact):
        out = np.zeros(max(self.m, 1), np.uint8)
        if lib().dpgo_pcm_solve(self._h, int(exact), out.ctypes.data_as(C.c_void_p)) < 0:
            raise RuntimeError("dpgo_pcm_solve failed")
        return out[:self.m].astype(bool)

    def solve_exact(self):
        """PCM::solveExact -> results(): one bool per measurement (a maximum clique)."""
        return self._solve(True)

    def solve_heuristic(self):
        """PCM::solveHeuristic -> results(): one bool per measurement (a clique)."""
        return self._solve(False)


def max_clique(A, exact=True):
    """Host max clique (dpgo_max_clique) of the 0/1 matrix A (A | A^T used, diagonal ignored): bool per vertex."""
    A = np.ascontiguousarray(np.asarray(A) != 0, np.uint8)
    m = A.shape[0]
    if A.shape != (m, m):
        raise ValueError("A must be square")
    out = np.zeros(max(m, 1), np.uint8)
    if lib().dpgo_max_clique(m, A.ctypes.data_as(C.c_void_p), int(bool(exact)), out.ctypes.data_as(C.c_void_p)) < 0:
        raise RuntimeError("dpgo_max_clique failed")
    return out[:m].astype(bool)


def pose_nodes(graph):
    """Node of every global pose id under the graph's contiguous partition."""
    off = np.asarray([graph.node_offset(a) for a in range(graph.num_nodes)])
    return np.searchsorted(off, np.arange(graph.num_poses), side="right") - 1


def pcm_inliers(graph, X, tolerance=0.2, weighted=False, exact=True, device=0):
    """PCM over every pair of nodes that shares edges: a keep-mask over all edges of the graph (intra-node edges
    are always kept; an inter-node edge is kept when it is in the clique of its pair).  graph.filter_edges(mask)
    gives the graph without the rejected closures."""
    I, J = graph.edges()[:2]
    node = pose_nodes(graph)
    ni, nj = node[I], node[J]
    keep = np.ones(graph.num_edges, bool)
    inter = ni != nj
    pairs = sorted(set(zip(np.minimum(ni, nj)[inter].tolist(), np.maximum(ni, nj)[inter].tolist())))
    pcm = PCM(device)
    for a, b in pairs:
        if pcm.update(graph, a, b, X, tolerance, weighted) == 0:
            continue
        ids = pcm.measurements()
        inl = pcm.solve_exact() if exact else pcm.solve_heuristic()
        keep[ids[~inl]] = False
    return keep


class EdgeSummary(C.Structure):
    """dpgo_edge_summary_t: F = F_intra + F_inter, the smallest weight, the inter-node edges and those with w < 1."""
    _fields_ = [("F", C.c_double), ("F_intra", C.c_double), ("F_inter", C.c_double), ("weight_min", C.c_double),
                ("num_inter", C.c_int), ("num_downweighted", C.c_int)]


class EdgeEval:
    """Per-edge residuals, loss values and loss weights of a whole graph at a global X, on the GPU (dpgo_edge_eval_*;
    the definitions are in include/dpgo_amd.h).  The edge records are uploaded once; run() uploads X and returns
    (s_rot, s_trans, rho, weight, EdgeSummary), arrays of num_edges doubles in graph order.  There is no CPU path:
    constructing one without a HIP device raises."""

    def __init__(self, graph, device=0):
        h = C.c_void_p()
        if lib().dpgo_edge_eval_create(graph._h, int(device), C.byref(h)) != 0:
            raise RuntimeError("dpgo_edge_eval_create failed (no HIP device?); there is no CPU path")
        self._h = h
        self.graph = graph
        self.m = graph.num_edges

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dpgo_edge_eval_free(self._h)
            self._h = None

    def run(self, X, loss=LOSS_NONE, loss_reg=0.25):
        X, ld = _fcol(X)
        out = [np.zeros(self.m) for _ in range(4)]
        s = EdgeSummary()
        if lib().dpgo_edge_eval_run(self._h, _dp(X), ld, int(loss), float(loss_reg), *[_dp(a) for a in out], C.byref(s)) != 0:
            raise ValueError("dpgo_edge_eval_run failed (a short X, an unknown loss, or a bad loss_reg)")
        return out[0], out[1], out[2], out[3], s

    def summary(self, X, loss=LOSS_NONE, loss_reg=0.25):
        """The summary alone: nothing but 40 bytes is read back."""
        X, ld = _fcol(X)
        s = EdgeSummary()
        if lib().dpgo_edge_eval_run(self._h, _dp(X), ld, int(loss), float(loss_reg), None, None, None, None, C.byref(s)) != 0:
            raise ValueError("dpgo_edge_eval_run failed (a short X, an unknown loss, or a bad loss_reg)")
        return s

    def kernel_ms(self):
        """Device time of the last run's kernels (HIP events around the two launches)."""
        ms = C.c_double()
        lib().dpgo_edge_eval_kernel_ms(self._h, C.byref(ms))
        return ms.value


def edge_eval_host(graph, X, loss=LOSS_NONE, loss_reg=0.25):
    """Debug, no GPU: the edge kernel's computation on the host, lane by lane in the device's order of summation
    (dpgo_debug_edge_eval_host).  Returns what EdgeEval.run returns."""
    X, ld = _fcol(X)
    out = [np.zeros(graph.num_edges) for _ in range(4)]
    s = EdgeSummary()
    if lib().dpgo_debug_edge_eval_host(graph._h, _dp(X), ld, int(loss), float(loss_reg), *[_dp(a) for a in out], C.byref(s)) != 0:
        raise ValueError("dpgo_debug_edge_eval_host failed (a short X, an unknown loss, or a bad loss_reg)")
    return out[0], out[1], out[2], out[3], s


def robust_edge_debug(graph, X, loss=LOSS_NONE, loss_reg=0.25):
    """Debug, no GPU: the per-edge arithmetic of the robust Hessian's kernels on the host (dpgo_debug_robust_edge_host).
    Returns (w, c, rows, ghat): the weights, the curvatures c = 2 rho'', the rows (m, 2, d + 1, d) of (M_e X)_i and
    (M_e X)_j (row 0 the translation's, then the rows of Y), and the tangent gradients (m, 2, dof) of the edge at i and j."""
    X, ld = _fcol(X)
    d, m = graph.d, graph.num_edges
    dof = _dof(d)
    w, c, rows, gh = np.zeros(m), np.zeros(m), np.zeros((m, 2, d + 1, d)), np.zeros((m, 2, dof))
    if lib().dpgo_debug_robust_edge_host(graph._h, _dp(X), ld, int(loss), float(loss_reg), _dp(w), _dp(c), _dp(rows), _dp(gh)) != 0:
        raise ValueError("dpgo_debug_robust_edge_host failed (a short X, an unknown loss, or a bad loss_reg)")
    return w, c, rows, gh


def ml_edge_debug(graph, X):
    """Debug, no GPU: the per-edge arithmetic of the maximum-likelihood kernels on the host (dpgo_debug_ml_edge_host).
    Returns a dict: r, wr (m, dof), chi2 (m), Ji, Jj (m, dof, dof: rows r, columns the pose's unknowns), grad (m, 2, dof:
    J_i' Omega r, J_j' Omega r), blocks (m, 4, dof, dof: the edge's terms of (i, i), (i, j), (j, i), (j, j)), near_pi."""
    X, ld = _fcol(X)
    m, dof = graph.num_edges, _dof(graph.d)
    o = {"r": np.zeros((m, dof)), "wr": np.zeros((m, dof)), "chi2": np.zeros(m), "Ji": np.zeros((m, dof, dof)),
         "Jj": np.zeros((m, dof, dof)), "grad": np.zeros((m, 2, dof)), "blocks": np.zeros((m, 4, dof, dof))}
    near = C.c_longlong(0)
    if lib().dpgo_debug_ml_edge_host(graph._h, _dp(X), ld, *[_dp(o[k]) for k in ("r", "wr", "chi2", "Ji", "Jj", "grad", "blocks")],
                                     C.byref(near)) != 0:
        raise ValueError("dpgo_debug_ml_edge_host failed (a short X, an edge outside the graph, or an information matrix of edge "
                         "... that is not symmetric positive definite: see stderr)")
    o["near_pi"] = near.value
    return o


def ml_gnc_edge_debug(graph, X, w):
    """Debug, no GPU: the per-edge arithmetic of `ml_gnc`'s weighted edge pass on the host (dpgo_debug_ml_gnc_edge_host) for
    the weights w (one per edge, each in [0, 1]).  Returns a dict: r, wr = w Omega r (m, dof), chi2 (m, unweighted), grad (m, 2,
    dof), Ji, Jj, Wi, Wj (m, dof, dof; W = w Omega J; the four are zero where w == 0), near_pi (over w > 0), near_pi_all."""
    X, ld = _fcol(X)
    m, dof = graph.num_edges, _dof(graph.d)
    w = np.ascontiguousarray(w, np.float64)
    if w.shape != (m,):
        raise ValueError("ml_gnc_edge_debug: w must have one entry per edge")
    o = {"r": np.zeros((m, dof)), "wr": np.zeros((m, dof)), "chi2": np.zeros(m), "grad": np.zeros((m, 2, dof))}
    jw = np.zeros((m, 4, dof, dof))
    near, near_all = C.c_longlong(0), C.c_longlong(0)
    if lib().dpgo_debug_ml_gnc_edge_host(graph._h, _dp(X), ld, _dp(w), *[_dp(o[k]) for k in ("r", "wr", "chi2", "grad")], _dp(jw),
                                         C.byref(near), C.byref(near_all)) != 0:
        raise ValueError("dpgo_debug_ml_gnc_edge_host failed (a short X, an edge outside the graph, a weight outside [0, 1], or an "
                         "information matrix that is not symmetric positive definite: see stderr)")
    o.update(Ji=jw[:, 0], Jj=jw[:, 1], Wi=jw[:, 2], Wj=jw[:, 3], near_pi=near.value, near_pi_all=near_all.value)
    return o


def robust_sens_edge_debug(graph, X, lam, loss=LOSS_NONE, loss_reg=0.25):
    """Debug, no GPU: the per-edge arithmetic of the robust sensitivities' kernels on the host
    (dpgo_debug_robust_sens_edge_host) for one adjoint `lam` (dof N by global pose, used as given).  Returns (sens, phi):
    (num_edges, 3 + dof) in NodeGroup.robust_sensitivity's order, and phi_e per edge."""
    X, ld = _fcol(X)
    dof, m = _dof(graph.d), graph.num_edges
    lam = np.ascontiguousarray(lam, np.float64)
    if lam.shape != (dof * graph.num_poses,):
        raise ValueError("robust_sens_edge_debug: lam must have dof N entries")
    sens, phi = np.zeros((m, 3 + dof)), np.zeros(m)
    if lib().dpgo_debug_robust_sens_edge_host(graph._h, _dp(X), ld, int(loss), float(loss_reg), _dp(lam), _dp(sens), _dp(phi)) != 0:
        raise ValueError("dpgo_debug_robust_sens_edge_host failed (a short X, an edge outside the graph, an unknown loss, or a bad "
                         "loss_reg)")
    return sens, phi


def verify_reweighted(graph, X, loss, loss_reg=0.25, eta=1e-3, tau=1e-6, max_iters=2000, precondition=True,
                      stop_on_negative=True, seed=0, refresh_every=50, max_factor_bytes=0, device=0):
    """The certificate of the RE-WEIGHTED problem at X (dpgo_graph_verify_reweighted): the loss weights w_e = w(s_e(X)) are
    frozen, the inter-node kappa_e, tau_e scaled by them, and NodeGroup.verify runs on a trivial-loss group of that graph.
    Returns (CertResult, x, CertFactor, EdgeSummary).  stationarity is the robust gradient norm.  CERT_PROVEN says that X is
    the global minimiser of its own quadratic surrogate -- a fixed point of an exact MM step -- NOT that it is the global
    minimum of the robust objective (include/dpgo_amd.h)."""
    X, ld = _fcol(X)
    o = _cert_args(X, "verify_reweighted", eta, tau, max_iters, precondition, stop_on_negative, refresh_every, seed)[0]
    res, f, s = CertResult(), CertFactor(), EdgeSummary()
    x = np.zeros(X.shape[0])
    if lib().dpgo_graph_verify_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), C.byref(o),
                                          int(max_factor_bytes), C.byref(res), C.byref(f), C.byref(s), _dp(x), x.shape[0]) != 0:
        raise RuntimeError("dpgo_graph_verify_reweighted failed (no HIP device, a short X, or a bad loss)")
    return res, x, f, s


def covariance_reweighted(graph, X, loss, loss_reg=0.25, anchor=0, pairs=None, max_bytes=0, device=0):
    """The covariances of the RE-WEIGHTED problem at X (dpgo_graph_covariance_reweighted), by verify_reweighted's recipe: the
    loss weights frozen at X, the inter-node edges scaled by them, NodeGroup.covariance on a trivial-loss group of that
    graph.  Returns (marginals, cross, CovResult, EdgeSummary).  This is the covariance of the MM surrogate at its fixed
    point, NOT of the robust objective (include/dpgo_amd.h)."""
    X, ld = _fcol(X)
    marg, cross, pair_args = _pairs_arg(pairs, graph.num_poses, _dof(graph.d))
    r, s = CovResult(), EdgeSummary()
    if lib().dpgo_graph_covariance_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), int(anchor),
                                              int(max_bytes), *pair_args, C.byref(r), C.byref(s)) != 0:
        raise RuntimeError("dpgo_graph_covariance_reweighted failed (no HIP device, a short X, a bad loss, or a pair that is no edge)")
    return marg, cross, r, s


def pair_covariance_reweighted(graph, X, loss, pairs, loss_reg=0.25, anchor=0, candidates=None, max_bytes=0, threshold=None,
                               device=0):
    """NodeGroup.pair_covariance for the RE-WEIGHTED problem at X (dpgo_graph_pair_covariance_reweighted), by
    covariance_reweighted's recipe and with its caveat.  Returns pair_covariance's dict with summary (EdgeSummary) added."""
    X, ld = _fcol(X)
    gated, joint, rel, gate, pair_args = _pair_cov_arg(graph.d, pairs, candidates)
    r, s = PairsResult(), EdgeSummary()
    if lib().dpgo_graph_pair_covariance_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), int(anchor),
                                                   int(max_bytes), *pair_args, C.byref(r), C.byref(s)) != 0:
        raise RuntimeError("dpgo_graph_pair_covariance_reweighted failed (no HIP device, a short X, a bad loss, a pose outside the "
                           "graph, or a candidate weight that is not positive)")
    out = pairs_output(joint, rel, gate, r, gated, threshold)
    out["summary"] = s
    return out


def joint_marginal_reweighted(graph, X, loss, keep, loss_reg=0.25, anchor=0, base=None, want_info=True, max_bytes=0, device=0):
    """NodeGroup.joint_marginal for the RE-WEIGHTED problem at X (dpgo_graph_joint_marginal_reweighted), by
    covariance_reweighted's recipe and with its caveat.  Returns joint_marginal's dict with summary (EdgeSummary) added."""
    X, ld = _fcol(X)
    cov, info, logdet, order, args = _marg_arg(graph.d, keep, base, want_info)
    r, s = MargResult(), EdgeSummary()
    if lib().dpgo_graph_joint_marginal_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), args[0], args[1],
                                                  int(anchor), args[2], int(bool(want_info)), int(max_bytes), _dp(cov), _dp(info),
                                                  _dp(logdet), C.byref(r), C.byref(s)) != 0:
        raise RuntimeError("dpgo_graph_joint_marginal_reweighted failed (no HIP device, a short X, a bad loss, or a bad pose list)")
    out = marg_output(cov, info, logdet, order, r, want_info)
    out["summary"] = s
    return out


def candidate_set_reweighted(graph, X, loss, pairs, candidates, loss_reg=0.25, anchor=0, budget=0, d2_max=0.0, want_joint=True,
                             want_cov=True, max_bytes=0, device=0):
    """NodeGroup.candidate_set for the RE-WEIGHTED problem at X (dpgo_graph_candidate_set_reweighted), by
    pair_covariance_reweighted's recipe and with its caveat.  Returns candidate_set's dict with summary (EdgeSummary) added."""
    X, ld = _fcol(X)
    a, head, tail = _cand_arg(graph.d, pairs, candidates, budget, want_joint, want_cov)
    r, s = CandResult(), EdgeSummary()
    if lib().dpgo_graph_candidate_set_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), *head, int(anchor),
                                                 a["budget"], float(d2_max), int(bool(want_joint)), int(max_bytes), *tail,
                                                 C.byref(r), C.byref(s)) != 0:
        raise RuntimeError("dpgo_graph_candidate_set_reweighted failed (no HIP device, a short X, a bad loss, a pose outside the "
                           "graph, a candidate that joins a pose to itself, or a weight that is not positive)")
    out = cand_output(a, r, want_joint)
    out["summary"] = s
    return out


def edge_reliability_reweighted(graph, X, loss, loss_reg=0.25, edges=None, anchor=0, method=0, max_bytes=0, device=0):
    """NodeGroup.edge_reliability for the RE-WEIGHTED problem at X (dpgo_graph_edge_reliability_reweighted), by
    covariance_reweighted's recipe and with its caveat: the records describe the MM surrogate, not the robust objective.  Returns
    edge_reliability's dict with summary (EdgeSummary) added."""
    X, ld = _fcol(X)
    records, rel, joint, edge_args = _rely_arg(graph, edges)
    r, s = RelyResult(), EdgeSummary()
    if lib().dpgo_graph_edge_reliability_reweighted(graph._h, int(device), _dp(X), ld, int(loss), float(loss_reg), int(anchor),
                                                    int(max_bytes), int(method), *edge_args, _dp(records), _dp(rel), _dp(joint),
                                                    C.byref(r), C.byref(s)) != 0:
        raise RuntimeError("dpgo_graph_edge_reliability_reweighted failed (no HIP device, a short X, a bad loss, an edge index "
                           "outside the graph, or an unknown method)")
    out = rely_output(graph.d, records, rel, joint, r)
    out["summary"] = s
    return out
