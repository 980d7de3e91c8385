/* dpgo_amd -- C ABI of the MI355X-native DPGO hot path.
 *
 * Drop-in boundary for the per-node MM / AMM inner step of the reference's
 * `dist_pgo` (MurpheyLab/DPGO).  Plain pointers and sizes only; the caller owns
 * host buffers, the library owns device memory behind opaque handles.  Every
 * function returns 0 on success and -1 on error (with a line on stderr), which
 * is the reference's own convention (`return -1` + LOG(ERROR), e.g.
 * C++/DPGO/include/DPGO/DPGOHash.h:43-47, C++/DPGO/include/DPGO/DPGO_utils.h:402-406).
 *
 * Matrices X are column-major with an explicit leading dimension, in the
 * reference layout: rows [0,n) translations t_i^T, rows [n + d i, n + d i + d)
 * the block R_i^T (C++/DPGO/include/DPGO/DPGOProblem.h:167-171).  The
 * conversion to the pose-contiguous device layout happens inside the library.
 *
 * A "group" is the set of nodes hosted by one GPU / one process; it replaces a
 * std::vector<std::shared_ptr<DPGOHash>> restricted to those nodes, and its
 * batched calls replace the driver's `for (alpha...) dpgo_hash[alpha]->...()`
 * loops (C++/examples/dist_pgo.cpp:455-462, 496-521).
 */
#ifndef DPGO_AMD_H
#define DPGO_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* DPGO::Options -- C++/DPGO/include/DPGO/DPGO_types.h:78-201: same names, same defaults, enums as their integer
 * values.  verbose prints one summary line per truncated-Newton refinement.  Not carried: user_function, log_iterates
 * (no effect on the iterates).
 * dpgo_group_create fails (-1) for what is not implemented: preconditioner IncompleteCholesky. */
typedef struct dpgo_options {
  int scheme;                 /* 0 = Scheme::MM, 1 = Scheme::AMM */
  double regularizer;
  double accepted_delta;
  double eta[2];
  double psi;
  double phi;
  int max_soft_restart_hits[2];
  int oscillation_cnt_period;
  int max_oscillations;
  int loss;                   /* 0 None, 1 Huber, 2 GemanMcClure, 3 Welsch */
  double loss_reg;
  int rescale;                /* Rescale (DPGO_types.h:43-46): 0 Static, 1 Dynamic (the reference default, :128) */
  int max_rescale_count;      /* DPGO_types.h:131 */
  double grad_norm_tol;
  double rel_func_decrease_tol;
  double stepsize_tol;
  int max_iterations;
  int max_iterations_accepted;
  double reg_Cholesky_precon_max_condition_number;
  double preconditioned_grad_norm_tol;
  int max_tCG_iterations;
  double STPCG_kappa;
  double STPCG_theta;
  int preconditioner;         /* Preconditioner (DPGO_types.h:35-40): 0 None, 1 Jacobi, 2 IncompleteCholesky,
                                 3 RegularizedCholesky (default) */
  int verbose;                /* DPGO_types.h:87: 0 (default) quiet; 1: a line per node and refinement on stdout */
} dpgo_options_t;

/* The scalar part of DPGOResult -- C++/DPGO/include/DPGO/DPGO_types.h:204-322. */
typedef struct dpgo_results {
  int updated;
  int iters;
  double gradFnorm;
  double fobjE;
  double Fk[2];
  double Gk;
  double Gkh;
  double fobj;                /* fobj[iters] */
  double f;                   /* f[iters] */
  double gamma;
  double s[2];                /* s[iters], s[iters+1] */
  int soft_restart_hits[2];
  int num_oscillations;
  int refined;                /* whether the last iterate() ran the TNT refinement */
  int tnt_status;             /* TNTStatus of that run (TNT.h:134-164), -1 if none */
  int tnt_inner_iterations;
  int restarts;
} dpgo_results_t;


typedef struct dpgo_graph dpgo_graph_t;
typedef struct dpgo_group dpgo_group_t;

/* Options() defaults, and the overrides of C++/examples/dist_pgo.cpp:103-120. */
void dpgo_options_default(dpgo_options_t *opt);
void dpgo_options_driver(dpgo_options_t *opt, int loss, int accelerated);

/* DPGO::read_g2o -- C++/DPGO/include/DPGO/DPGO_utils.h:49-51, C++/DPGO/src/DPGO_utils.cpp:140-202. */
int dpgo_read_g2o(const char *filename, int num_nodes, dpgo_graph_t **out);
/* The same partition applied to measurements already in memory (tail I, head J global pose ids,
 * R row-major d x d, t d). */
int dpgo_graph_from_edges(int d, int num_poses, int m, const int *I, const int *J, const double *R,
                          const double *t, const double *kappa, const double *tau, int num_nodes,
                          dpgo_graph_t **out);
void dpgo_graph_free(dpgo_graph_t *g);
int dpgo_graph_info(const dpgo_graph_t *g, int *d, int *num_poses, int *num_nodes, int *num_edges);
/* copies the parsed measurements (file order); any output pointer may be NULL */
int dpgo_graph_edges(const dpgo_graph_t *g, int *I, int *J, double *R, double *t, double *kappa, double *tau);
/* The measurements' full information matrices, which the maximum-likelihood refinement (dpgo_group_ml_polish, below) uses.
 * A graph read from a file keeps every edge's Omega (the file's upper triangle, symmetrised; dof x dof, dof = d + d (d - 1) / 2,
 * translation first, then rotation); dpgo_graph_from_edges keeps none; dpgo_graph_from_edges_info is its sibling with
 * info: m x dof^2 doubles, row-major, used as given.  kappa and tau are not derived from info: both are the caller's.
 * dpgo_graph_edge_information: out (num_edges x dof^2, or NULL) <- every edge's Omega, for a graph without one Omega_iso =
 * diag(tau I_d, 2 kappa I); *has (or NULL) <- whether the graph keeps its own.  dpgo_graph_filter_edges carries Omega along,
 * dpgo_graph_scale_edges carries it along times w_e. */
int dpgo_graph_from_edges_info(int d, int num_poses, int m, const int *I, const int *J, const double *R, const double *t,
                               const double *kappa, const double *tau, const double *info, int num_nodes, dpgo_graph_t **out);
int dpgo_graph_edge_information(const dpgo_graph_t *g, double *out, int *has);
/* DPGOProblem::n() / m() -- C++/DPGO/include/DPGO/DPGOProblem.h:241-248 (host only) */
int dpgo_graph_node_sizes(const dpgo_graph_t *g, int node, int *n0, int *n1, int *m0, int *m1);
/* neighbour ordering of generate_data_info (C++/DPGO/src/DPGO_utils.cpp:400-418): n1 (node, pose) pairs */
int dpgo_graph_node_neighbours(const dpgo_graph_t *g, int node, int *nbr_node, int *nbr_pose);
/* first global pose id of a node (g_index[node].begin()->second, dist_pgo.cpp:470) */
int dpgo_graph_node_offset(const dpgo_graph_t *g, int node);
/* Boundary-exchange plan of a group of nodes (host only): the (node, pose) keys it exports to and
 * imports from nodes outside the group, both sorted.  counts[0] = exported, counts[1] = imported; the
 * key arrays may be NULL to query the counts.  (sent_ / recv_ of C++/DPGO/src/DPGO_utils.cpp:428-435.) */
int dpgo_graph_exchange_plan(const dpgo_graph_t *g, const int *node_ids, int num_local, int *sent_nodes,
                             int *sent_poses, int *recv_nodes, int *recv_poses, int *counts);
/* DPGOProblem::index() / sent() / recv() -- C++/DPGO/include/DPGO/DPGOProblem.h:212-225 (host only): the entries
 * {(node, pose) -> (block, k)} of the map `which` (0 index, 1 sent, 2 recv), in map order.  Arrays may be NULL
 * to query *count. */
int dpgo_graph_node_maps(const dpgo_graph_t *g, int node, int which, int *nodes, int *poses, int *block, int *local,
                         int *count);
/* Result format: VERTEX_SE2 / VERTEX_SE3:QUAT lines from X ((d+1)N x d; NULL: edges only) followed
 * by the graph's EDGE_* lines with the isotropic information the loader's formulas invert. */
int dpgo_write_g2o(const dpgo_graph_t *g, const double *X, int ld, const char *filename);
/* Centralised chordal initialisation -- C++/examples/dist_pgo.cpp:416-444
 * (C++/SESync/src/SESync_utils.cpp:573-652).  Host, set-up only.  X: (d+1)N x d. */
int dpgo_chordal_initialization(const dpgo_graph_t *g, double *X, int ld);

/* Distributed chordal initialisation -- the `--dist_init true` branch of C++/examples/dist_pgo.cpp:144-416 on
 * C++/DChordal (DChordalReduced_R, DChordal_R, DChordalReduced_t, DChordal_t; DChordal.cpp:79-152,
 * DChordalProblem.h:128-246, DChordal_utils.cpp:67-1204).  The two sparse stages run on the group's GPU, the two
 * reduced ones (one d x d block / one translation per node) on the host.  Every node of the graph must be in the
 * group, in order.  opts: DChordal::Options::reg_G, the driver's stage schedule, and the length of the stage-0
 * stand-in (the reference's stage 0 is a per-node SE-Sync solve, out of scope: here chordal initialisation of the
 * node's own subgraph + local_iters refined MM-PGO iterations).  X_local (optional): stage-0 poses of every node in
 * the global layout.  X: (d+1)N x d result.  objectives (optional, capacity *num_objectives on entry): 0.5 sum |B X +
 * b|^2 sampled every 20 iterations through the four stages (what the driver prints, :206-210). */
typedef struct dpgo_dchordal_options {
  int iters[4];      /* 100, 400, 150, 250 */
  int local_iters;   /* 30 */
  double reg_G;      /* 1e-12 (DChordal_types.h:50) */
} dpgo_dchordal_options_t;
void dpgo_dchordal_options_default(dpgo_dchordal_options_t *opt);
int dpgo_group_dist_chordal_initialization(dpgo_group_t *grp, const dpgo_dchordal_options_t *opt, const double *X_local,
                                           int ld_local, double *X, int ld, double *objectives, int *num_objectives);

/* DPGOHash(node, measurements, options) for every node in node_ids -- C++/DPGO/src/DPGOHash.cpp:11-18,
 * C++/DPGO/src/DPGOProblem.cpp:11-125.  Fails (-1) when no HIP device is present: there is no CPU path. */
int dpgo_group_create(const dpgo_graph_t *g, const int *node_ids, int num_local, const dpgo_options_t *opt,
                      int device, dpgo_group_t **out);
void dpgo_group_free(dpgo_group_t *grp);

/* DPGOHash::initialize -- C++/DPGO/src/DPGOHash.cpp:20-43.  X: (d+1)(n0+n1) x d. */
int dpgo_group_initialize(dpgo_group_t *grp, int local, const double *X, int ld);
/* Split a global X over the nodes and fill neighbour rows -- dist_pgo.cpp:435-446 + DPGO::communicate. */
int dpgo_group_initialize_global(dpgo_group_t *grp, const double *X, int ld);
/* DPGOHash::update / iterate -- C++/DPGO/src/DPGOHash.cpp:84-228, 583-628.  locals == NULL: every node. */
int dpgo_group_update(dpgo_group_t *grp, const int *locals, int n);
int dpgo_group_iterate(dpgo_group_t *grp, const int *locals, int n);
/* DPGOHash::communicate -- C++/DPGO/include/DPGO/DPGOHash.h:28-86 -- for neighbours hosted by this group. */
int dpgo_group_communicate_local(dpgo_group_t *grp);
/* One pass of the driver's loop body -- C++/examples/dist_pgo.cpp:496-521: iterate() of every node of the group, the
 * boundary exchange (`comm`: a communicator made by dpgo_comm_create for this group, or NULL when every neighbour is hosted
 * here), communicate(), update() of every node -- in one call, so that a host in another language does not put its own
 * call overhead between the launches. */
struct dpgo_comm;
int dpgo_group_step(dpgo_group_t *grp, struct dpgo_comm *comm);
/* DPGOHash::receive -- C++/DPGO/src/DPGOHash.cpp:45-82: one message per neighbour node beta, a
 * ((d+1) |recv[beta]|) x d matrix [translation rows ; rotation rows] with the poses in the order of
 * recv[beta].  dpgo_group_send builds the message node `local` owes node beta (the poses of sent[beta],
 * C++/DPGO/src/DPGO_utils.cpp:428-435) from its current Xk.  Host matrices, column-major. */
int dpgo_group_message_sizes(const dpgo_group_t *grp, int local, int beta, int *num_send, int *num_recv);
int dpgo_group_send(const dpgo_group_t *grp, int local, int beta, double *msg, int ld);
int dpgo_group_receive(dpgo_group_t *grp, int local, int beta, const double *msg, int ld);
/* AMM-PGO* -- DPGOStar::{initialize, update, iterate} (C++/DPGO/src/DPGOStar.cpp:107-213; per-node
 * helpers :215-711); communicate() is dpgo_group_communicate_local (+ the boundary exchange between groups).
 * Either every node of the graph is in the group, or the groups are connected by dpgo_group_set_collectives
 * (the master's global objective is the sum of the per-node device reductions over all groups).  Loop:
 * star_initialize(X); repeat { star_update; star_iterate; communicate_local }.
 * star_state: F (running average, :210), fobj = F(X_k+1), fobjh = F(X_k+1/2), branches bit 0 = plain
 * proximal redo (:149-155), bit 1 = MM redo (:159-169), bit 2 = proximal-rotation fallback (:171-192). */
/* AMM-PGO* with the nodes spread over several groups (one process per GPU): the caller lends the library two
 * collectives.  allgather(user): all-gather the registered device buffer `send` (stride * (d+1)*d doubles, the
 * layout of dpgo_group_pack_sent) into `gathered` (the layout given to dpgo_group_set_recv_layout), ordered on
 * dpgo_group_stream().  allreduce(user, vals, n): in-place sum of n host doubles over all groups; every group
 * must get bit-identical results (they steer the same branches: DPGOStar.cpp:147-192).  Both return 0 on success. */
typedef int (*dpgo_allgather_fn)(void *user);
typedef int (*dpgo_allreduce_fn)(void *user, double *vals, int n);
int dpgo_group_set_collectives(dpgo_group_t *grp, void *send, void *gathered, dpgo_allgather_fn allgather,
                               dpgo_allreduce_fn allreduce, void *user);
int dpgo_group_star_initialize(dpgo_group_t *grp, const double *X, int ld);
int dpgo_group_star_update(dpgo_group_t *grp);
int dpgo_group_star_iterate(dpgo_group_t *grp);
int dpgo_group_star_state(const dpgo_group_t *grp, double *F, double *fobj, double *fobjh, int *branches);
/* Boundary exchange with other groups (the message of DPGOHash::receive, DPGOHash.cpp:45-82):
 * pack this group's exported poses into a device buffer of num_sent * (d+1)*d doubles, all-gather
 * the buffers of all groups (RCCL), then unpack.  Keys are (node, pose).
 * dpgo_group_unpack_recv is LAZY for the robust losses (round 6): the neighbour rows stay in `device_gathered` until the
 * group next looks at them -- the next dpgo_group_update reads them from there inside its inter-edge pass and stores them
 * into Xk on the way (no unpack kernel); any other reader (dpgo_group_get_Xk, ...) gets the plain indexed copy first.  The
 * buffer must therefore stay untouched until that update (or any call that reads the group's state) has been made;
 * everything is ordered on dpgo_group_stream(). */
int dpgo_group_num_sent(const dpgo_group_t *grp);
int dpgo_group_sent_keys(const dpgo_group_t *grp, int *nodes, int *poses);
int dpgo_group_set_recv_layout(dpgo_group_t *grp, int nranks, int stride, const int *counts, const int *nodes,
                               const int *poses);
int dpgo_group_pack_sent(dpgo_group_t *grp, void *device_buffer);
int dpgo_group_unpack_recv(dpgo_group_t *grp, const void *device_gathered);

/* DPGOStar::evaluate_f / evaluate_grad -- C++/DPGO/src/DPGOStar.cpp:713-829 -- at an ARBITRARY global X
 * ((d+1)N x d); the optimizer state is not touched.  *F and *grad_sqnorm (= |grad F|^2, Riemannian) are sums over
 * the nodes of this group -- over all groups when collectives are set (dpgo_group_set_collectives / dpgo_comm_create);
 * the driver prints 2 F and 2 sqrt(grad_sqnorm) (dist_pgo.cpp:477-481).  grad (optional, (d+1)N x d, leading
 * dimension ldg): the rows of this group's own poses are written.  Any output pointer may be NULL. */
int dpgo_group_evaluate(dpgo_group_t *grp, const double *X, int ld, double *F, double *grad_sqnorm, double *grad,
                        int ldg);
/* DPGOHash::set_options / options -- C++/DPGO/include/DPGO/DPGOHash.h:91-96.  Fields that are part of the problem
 * built at construction (loss, loss_reg, regularizer, rescale, preconditioner) must keep their values (-1). */
int dpgo_group_set_options(dpgo_group_t *grp, const dpgo_options_t *opt);
int dpgo_group_get_options(const dpgo_group_t *grp, dpgo_options_t *opt);

/* ---- the exchange between GPUs: RCCL behind the C ABI (one process per GPU; replaces the in-process copies of
 * DPGOHash::communicate, C++/DPGO/include/DPGO/DPGOHash.h:28-86, and the master's sums of DPGOStar.cpp:147-192).
 * dpgo_comm_unique_id: ncclGetUniqueId on one rank; the caller carries the 128 bytes to the others (file, socket,
 *   MPI, torch.distributed -- any channel).
 * dpgo_comm_create: ncclCommInitRank + the exchange lay-out (the ranks all-gather their exported (node, pose) keys);
 *   also connects the group's AMM-PGO* / global-evaluation collectives (dpgo_group_set_collectives) to RCCL.
 * dpgo_comm_exchange: communicate() for neighbours hosted by other ranks; returns at once.  Neighbour to neighbour (the
 *   default with several ranks): ncclGroupStart, one ncclSend + ncclRecv per real neighbour, ncclGroupEnd on the GROUP's own
 *   stream -- the pack has ridden on the tail of dpgo_group_iterate, the unpack is the next dpgo_group_update's inter-edge
 *   pass reading the receive buffer (round 6; on a stream of its own the exchange paid two event hand-overs to hide one
 *   9 us kernel: profiles/r06_exchange_streams.txt).  All-gather (the fallback): pack, ncclAllGather, unpack on the
 *   communicator's own stream; the group's next update() joins it after queueing the part of the surrogate build that
 *   needs no neighbour data.  Call after dpgo_group_iterate, every rank, every iteration.
 * dpgo_comm_allreduce_sum: in-place sum of n host doubles over the ranks (bit-identical on every rank).
 * The library binds RCCL at run time (librccl.so.1); these calls return -1 when it cannot be loaded. */
typedef struct dpgo_comm dpgo_comm_t;
int dpgo_comm_unique_id(void *id128);
int dpgo_comm_create(dpgo_group_t *grp, int rank, int nranks, const void *id128, dpgo_comm_t **out);
void dpgo_comm_free(dpgo_comm_t *comm);
int dpgo_comm_exchange(dpgo_comm_t *comm);
int dpgo_comm_allreduce_sum(dpgo_comm_t *comm, double *vals, long n);
int dpgo_comm_barrier(dpgo_comm_t *comm);
/* How dpgo_comm_exchange moves the boundary poses: 1 = neighbour to neighbour (grouped ncclSend / ncclRecv, the default with
 * several ranks once its self-check passed on every rank), 0 = all-gather of fixed-size buffers; -1 on error. */
int dpgo_comm_exchange_kind(const dpgo_comm_t *comm);
/* Bytes this rank hands to RCCL per dpgo_comm_exchange (neighbour to neighbour: the records its peers need; all-gather: one
 * padded block); -1 on error.  Reported per rank by bench.py's N > 1 line. */
long dpgo_comm_bytes_sent(const dpgo_comm_t *comm);
/* Measurement hooks (bench.py --emulate-world N --force-exchange; no counterpart in the reference, whose "exchange" is a
 * memory copy, C++/DPGO/include/DPGO/DPGOHash.h:28-86):
 * dpgo_comm_self_exchange: on a communicator of ONE rank, dpgo_comm_exchange from now on runs the neighbour-to-neighbour path
 *   in its steady state with the rank as its own peer (the pack on the tail of iterate(), ncclGroupStart, ncclSend + ncclRecv
 *   of every exported record, ncclGroupEnd on the group's stream; what arrives -- the rank's own rows -- is not unpacked, the
 *   trajectory stays that of the run without an exchange): what that path costs an iteration, short of the wire;
 * dpgo_comm_enable_timing / dpgo_comm_exchange_time: mean time in microseconds between an event recorded in front of the
 *   exchange ("the iterate is final") and one behind it ("the neighbour rows have arrived"), over the exchanges since timing
 *   was enabled. */
int dpgo_comm_self_exchange(dpgo_comm_t *comm);
/* ... the same for a group whose neighbours NO rank hosts (one rank of an N-GPU run emulated on one GPU): a communicator of
 * one rank without the exchange lay-out, serving dpgo_comm_exchange in the self-exchange mode only */
int dpgo_comm_create_self(dpgo_group_t *grp, dpgo_comm_t **out);
int dpgo_comm_enable_timing(dpgo_comm_t *comm);
int dpgo_comm_exchange_time(dpgo_comm_t *comm, double *mean_us, long *count);
/* Test hook: the grouped ncclSend / ncclRecv path of dpgo_comm_exchange on a communicator of ONE rank that is its own peer
 * (legal inside ncclGroupStart / End): every row `grp` exports travels pack kernel -> group call -> unpack kernel on the
 * communicator's stream (the form of the creation-time check), on records that carry their own keys.  `grp` may host any subset of the nodes.  0 = every record
 * arrived in its row and no other row was touched; -1 otherwise (also when the group exports nothing). */
int dpgo_debug_comm_p2p_self(dpgo_group_t *grp);
/* The same pack / unpack on host matrices (no GPU needed; what a host-staged transport or a test uses): records
 * of the poses a group exports, in key order, from a global X ((d+1)N x d) into buf (count x (d+1)d doubles,
 * [t | rows of R^T] per pose); and the neighbour rows of node `node` ((d+1)(n0+n1) x d matrix Z, DPGOHash::initialize
 * lay-out) from the gathered buffers of all ranks (slot of key k of rank r = r * stride + k, as in
 * dpgo_group_set_recv_layout).  Return the number of poses written, -1 on error. */
int dpgo_host_pack_sent(const dpgo_graph_t *g, const int *node_ids, int num_local, const double *X, int ld, double *buf);
int dpgo_host_unpack_recv(const dpgo_graph_t *g, const int *node_ids, int num_local, int node, int nranks, int stride,
                          const int *counts, const int *nodes, const int *poses, const double *gathered, double *Z,
                          int ldz);

/* results().Xk / results().Xak -- DPGO_types.h:207-214 */
int dpgo_group_get_Xk(const dpgo_group_t *grp, int local, double *X, int ld);
int dpgo_group_get_Xak(const dpgo_group_t *grp, int local, double *X, int ld);
/* gather X^alpha into the global X -- dist_pgo.cpp:502-511 */
int dpgo_group_scatter_global(const dpgo_group_t *grp, double *X, int ld);
int dpgo_group_results(const dpgo_group_t *grp, int local, dpgo_results_t *out);
int dpgo_group_node_id(const dpgo_group_t *grp, int local);
int dpgo_group_sync(const dpgo_group_t *grp);
void *dpgo_group_stream(const dpgo_group_t *grp);   /* hipStream_t all work is enqueued on */

/* ---- measurement hooks (bench.py) --------------------------------------------------------
 * Per-launch timing of every kernel family with HIP events on the launch stream.  Off by default. */
int dpgo_prof_enable(int on);
int dpgo_prof_num_kinds(void);
const char *dpgo_prof_kind_name(int kind);
int dpgo_prof_collect(double *ms, double *bytes, long *count);   /* arrays of dpgo_prof_num_kinds() */
/* for the fused passes (k_inter, k_proximal): the bytes of every operand they move, counted one by one (0 for the others) */
int dpgo_prof_collect_operands(double *operand_bytes);
/* size of the two multifrontal factors: dense front entries and number of tree levels */
int dpgo_group_solver_stats(const dpgo_group_t *grp, long *nnz_tt, long *nnz_rr, int *levels_tt, int *levels_rr);
/* The branch-free segments of an iteration (C++/examples/dist_pgo.cpp:496-521: iterate, update) go to the GPU as replays of
 * captured HIP graphs where the host's launch rate would bound the group (DPGO_ITER_GRAPH=0 / 1 forces it off / on):
 * segments replayed, graphs captured, segments launched eagerly since the group was created. */
int dpgo_group_graph_stats(const dpgo_group_t *grp, long *replays, long *captures, long *eager);

/* ---- PCM: pairwise consistency maximisation (outlier rejection for inter-node loop closures) ----------------
 * DPGO::PCM -- C++/DPGO/include/DPGO/PCM.h, C++/DPGO/src/PCM.cpp:5-235.  For two nodes alpha != beta the measurement
 * list is the graph's alpha-beta edges (either direction) in graph edge order (dpgo_graph_edges order); X is the
 * GLOBAL iterate ((d+1)N x d, column-major, leading dimension ld), not the reference's two-node stacked X with its
 * index / num_s offsets (both pick the same poses).  The m x m consistency test runs on the device in fp64; the max
 * clique on the host.  Deviations: alpha == beta or a node out of range returns -1 (the reference would run on
 * alpha's intra-node edges); nothing calls exit(); rounding is not Eigen's, so only decisions away from the
 * tolerance are promised to match. */
typedef struct dpgo_pcm_options {
  double tolerance;   /* PCM.h:14, 0.2 */
  int weighted;       /* PCM.h:15, 0: kappa = tau = 1; 1: the pair's means of the edges' kappa and tau */
} dpgo_pcm_options_t;
typedef struct dpgo_pcm dpgo_pcm_t;
void dpgo_pcm_options_default(dpgo_pcm_options_t *opt);
/* PCM() (PCM.h:27-31) on HIP device `device`; -1 when there is no device (there is no CPU path). */
int dpgo_pcm_create(int device, dpgo_pcm_t **out);
void dpgo_pcm_free(dpgo_pcm_t *pcm);
/* PCM::update (PCM.cpp:5-235): returns m (0 for a pair without common edges), -1 on error (alpha == beta, a node out
 * of range, X NULL or ld < (d+1)N, m > 65536).  opts NULL: the defaults. */
int dpgo_pcm_update(dpgo_pcm_t *pcm, const dpgo_graph_t *g, int alpha, int beta, const double *X, int ld,
                    const dpgo_pcm_options_t *opts);
/* PCM::measurements (PCM.h:39): the m measurements as edge indices of the graph */
int dpgo_pcm_measurements(const dpgo_pcm_t *pcm, int *edge_ids);
/* PCM::adjancecy_matrix (PCM.h:37): the m x m 0/1 matrix (symmetric, diagonal 1) */
int dpgo_pcm_adjacency(const dpgo_pcm_t *pcm, unsigned char *dense);
/* Debug: the m x m pair errors of PCM.cpp:226-228 (row-major, symmetric, diagonal 0); m <= 4096 */
int dpgo_pcm_errors(dpgo_pcm_t *pcm, double *E);
/* PCM::solveExact / solveHeuristic (PCM.cpp:232-246) -> results() (PCM.h:41): inlier[k] = 1 for the members of the
 * clique found over the m measurements.  Returns the clique size. */
int dpgo_pcm_solve(dpgo_pcm_t *pcm, int exact, unsigned char *inlier);
/* Host only (no device): maximum clique (exact != 0) or the greedy heuristic on an m x m 0/1 matrix (row-major; the
 * symmetric matrix A | A^T is used, the diagonal is ignored).  out[k] = 1 for the members; returns the size. */
int dpgo_max_clique(int m, const unsigned char *dense, int exact, unsigned char *out);
/* The same poses and partition as g with only the edges e for which keep[e] != 0 (in order): how a caller drops the
 * closures PCM rejected before building groups.  -1 if no edge is kept. */
int dpgo_graph_filter_edges(const dpgo_graph_t *g, const unsigned char *keep, dpgo_graph_t **out);

/* ---- solution certificate: is the point the optimiser stopped at the global minimum? -------------------------
 * The reference answers this in its SE-Sync tree: SESyncProblem::compute_Lambda_blocks / verify_solution
 * (C++/SESync/src/SESyncProblem.cpp:375-468) and fast_verification (C++/SESync/src/SESync_utils.cpp:721-830) with LOBPCG
 * (C++/Optimization/include/Optimization/LinearAlgebra/LOBPCG.h:131-337).  X is the GLOBAL iterate ((d+1)N x d,
 * column-major, rows 0..N-1 translations, rows N + d p + r the rows of Y_p = R_p^T; DPGOProblem.h:167-171), M the data
 * matrix of the trivial loss (construct_data_matrix, DPGO_utils.cpp:440-718; F = 1/2 tr(X^T M X)).
 *   Lambda_p = 1/2 (P + P^T), P = (M X)[rows of Y_p] (X[rows of Y_p])^T           (SESyncProblem.cpp:375-395)
 *   S = M - blkdiag(0_N, Lambda_0, ..., Lambda_{N-1})                              (:444-447)
 * The search is LOBPCG on S with block size d, basis [V W P], on the device (fast_verification STEP 2, :765-826): |S| is
 * estimated on a Gaussian block (LOBPCG.h:199-214), column 0 has converged when r_0 <= tau (|S|_est + |theta_0|) |x_0|
 * (:298-307), and with stop_on_negative the search ends at once when theta_0 < -eta / 2 (SESync_utils.cpp:775-793).
 * `theta` and `residual` are recomputed from ONE fresh product S x of the returned unit vector x (theta = x^T S x,
 * residual = |S x - theta x|) and `status` is decided from them:
 *   DPGO_CERT_NEGATIVE     theta < -eta / 2: x PROVES lambda_min(S) < -eta / 2, X is not certified;
 *   DPGO_CERT_NONNEGATIVE  otherwise, and residual <= tau (|S|_est + |theta|).  This is EVIDENCE, NOT PROOF: a converged
 *                          Ritz pair need not be the smallest one.  The proof is a Cholesky factorisation of
 *                          S + eta I (STEP 1, :731-754): dpgo_group_cert_factor / dpgo_group_verify below;
 *   DPGO_CERT_UNDECIDED    max_iters reached without either.
 * `stationarity` is |S X|_F, the norm of the Riemannian gradient at X: the certificate only means something at a
 * critical point.  Deviations: the block size is fixed to d (a block IS a pose-record array); the preconditioner is
 * block Jacobi on the (d+1) x (d+1) diagonal blocks of M where the reference uses ILDL (STEP 3); trivial loss only -- a
 * group created with a robust loss returns -1 (create a second group with loss = 0 (None) and max_iterations = 0, which
 * skips the optimiser's factorisation -- at a ROBUST solution that group answers another question; its certificate is
 * dpgo_graph_verify_reweighted below); the group must host every node of the graph (-1 otherwise); rounding is not
 * Eigen's.  The optimiser's state is untouched. */
#define DPGO_CERT_UNDECIDED 0
#define DPGO_CERT_NONNEGATIVE 1
#define DPGO_CERT_NEGATIVE 2
typedef struct dpgo_cert_options {
  double eta;            /* min_eig_num_tol, C++/SESync/include/SESync/SESync.h:88, 1e-3 */
  double tau;            /* LOBPCG.h:138, 1e-6 */
  int max_iters;         /* 2000 */
  int precondition;      /* 1: block Jacobi */
  int stop_on_negative;  /* 1 */
  int refresh_every;     /* 50: S V and S P by real products every so many iterations; 0: never */
  unsigned long long seed;   /* of the Gaussian blocks (the norm estimate's, and the initial block when V0 is NULL) */
} dpgo_cert_options_t;
typedef struct dpgo_cert_result {
  int status, iterations, restarts;   /* restarts: Rayleigh-Ritz steps that dropped P (mass matrix pivot < 1e-12) */
  double theta, residual, S_norm_est, stationarity;
} dpgo_cert_result_t;
void dpgo_cert_options_default(dpgo_cert_options_t *opt);
/* fast_verification STEP 2 (SESync_utils.cpp:765-826).  V0: the initial block, (d+1)N x d, leading dimension ldv0, or
 * NULL (seeded Gaussians); x: receives the unit vector, (d+1)N entries, ldx >= (d+1)N, or NULL.  -1 on bad arguments. */
int dpgo_group_certify(dpgo_group_t *grp, const double *X, int ld, const dpgo_cert_options_t *opts, const double *V0,
                       int ldv0, dpgo_cert_result_t *result, double *x, int ldx);
/* compute_Lambda_blocks (SESyncProblem.cpp:375-395): Lambda receives N blocks d x d, row-major, by global pose */
int dpgo_group_cert_lambda(dpgo_group_t *grp, const double *X, int ld, double *Lambda);
/* SV = S(X) V, V and SV (d+1)N x d in the layout of X (the operator of verify_solution, :444-447, alone) */
int dpgo_group_cert_apply(dpgo_group_t *grp, const double *X, int ld, const double *V, int ldv, double *SV, int ldsv);
/* ---- the proof: fast_verification STEP 1 (SESync_utils.cpp:731-754), a Cholesky factorisation of S + eta I ------------
 * The factorisation exists exactly when the matrix is positive definite, so its success proves lambda_min(S) > -eta and a
 * non-positive pivot proves lambda_min(S) <= -eta.  S + eta I is written on the device as a CSR matrix on the unknowns
 * (d+1) p + r (pose p; r = 0 the translation, r = 1..d the rows of Y_p -- S acts alike on every column, so the matrix is
 * (d+1)N x (d+1)N), one explicit dense (d+1) x (d+1) block per pair of poses M couples, and factored by the library's
 * multifrontal Cholesky (nested dissection of the pose graph, MFMA fronts) in a factor-only mode: nothing is solved.
 * The symbolic analysis runs first, on the host, once per group; if it predicts more device memory than
 * max_factor_bytes (when > 0) or than half of what hipMemGetInfo reports free, nothing is allocated and the outcome is
 * DPGO_CERT_FACTOR_SKIPPED with the predicted sizes filled in.  A non-positive pivot is an outcome, not an error: nothing
 * is printed, and the next call factors again (the analysis and the device state do not depend on the values).
 *
 * What DPGO_CERT_PROVEN means.  It is a floating-point factorisation, as in the reference: its success proves that
 * S + eta I + E is positive definite for some E with |E|_2 of the order n^(3/2) u |S|_2 (Higham, Accuracy and Stability
 * of Numerical Algorithms, thm 10.7; n = (d+1)N, u = 2^-53), i.e. lambda_min(S) > -eta - |E|.  pivot_min, the smallest
 * pivot d_kk, bounds lambda_min(S + eta I) from ABOVE (pivots are diagonal entries of Schur complements), so a tiny
 * pivot_min says how close the call was.  And it says "X is a global minimum" ONLY where `stationarity` = |S X|_F is
 * small: S is built from X whether or not X is a critical point.  The warning example is sphere2500's chordal
 * initialisation on 4 nodes: lambda_min(S) = -5.65e-4, so eta = 1e-3 gives PROVEN -- at a point whose gradient norm
 * |S X|_F is 265 and which is nowhere near a minimum (eta = 1e-5 gives NOT_PD there).  Read both numbers.
 * Same restrictions as dpgo_group_certify (trivial loss, a group that hosts every node); the optimiser's state is
 * untouched. */
#define DPGO_CERT_PROVEN 3            /* only dpgo_group_verify returns it */
#define DPGO_CERT_FACTOR_NOT_PD 0
#define DPGO_CERT_FACTOR_PD 1
#define DPGO_CERT_FACTOR_SKIPPED 2
typedef struct dpgo_cert_factor {
  int outcome, fronts, levels, max_front;   /* fronts / tree levels / largest front (rows) of the elimination tree */
  long long factor_entries, factor_bytes;   /* sum (w + u) w over the fronts; device bytes of the numeric phase (every front
                                               matrix at once, the value array, the maps): both predicted by the analysis */
  double eta, pivot_min, pivot_max;         /* the pivot range of the fronts that factored (all of them for PD) */
  double stationarity;                      /* |S X|_F */
  double symbolic_s, numeric_s;             /* host seconds: the analysis (0 after a group's first call); matrix + factorisation */
} dpgo_cert_factor_t;
/* STEP 1 alone (SESync_utils.cpp:731-754).  eta: any finite shift.  -1 on bad arguments or a device error. */
int dpgo_group_cert_factor(dpgo_group_t *grp, const double *X, int ld, double eta, long long max_factor_bytes,
                           dpgo_cert_factor_t *factor);
/* fast_verification (SESync_utils.cpp:721-830): STEP 1 with opts->eta, then STEP 2 only when it did not succeed.
 *   FACTOR_PD       status = DPGO_CERT_PROVEN; the search does not run (iterations = 0, theta = residual = 0, x untouched),
 *                   stationarity is filled;
 *   FACTOR_NOT_PD   the search of dpgo_group_certify as it is (:756-826).  NEGATIVE stays NEGATIVE; a search that comes back
 *                   NONNEGATIVE has just been refuted by the factorisation and is returned as UNDECIDED, theta and
 *                   residual kept;
 *   FACTOR_SKIPPED  the search's own status, unchanged: dpgo_group_certify's answer, named as such by factor->outcome.
 * Arguments as for dpgo_group_certify. */
int dpgo_group_verify(dpgo_group_t *grp, const double *X, int ld, const dpgo_cert_options_t *opts, long long max_factor_bytes,
                      const double *V0, int ldv0, dpgo_cert_result_t *result, double *x, int ldx, dpgo_cert_factor_t *factor);
/* Debug: the matrix that is factored, S + eta I, read back from the device value array of the factorisation: CSR with
 * (d+1)N + 1 row pointers on the unknowns (d+1) g + r of the GLOBAL poses g, every stored block dense (structural zeros
 * explicit), *nnz = (d+1)^2 blocks.  With ptr = col = val = NULL only *nnz is set; otherwise cap >= *nnz. */
int dpgo_group_cert_matrix(dpgo_group_t *grp, const double *X, int ld, double eta, int *ptr, int *col, double *val, long long cap,
                           long long *nnz);
/* ---- per-edge residuals, loss values and loss weights; the certificate of the re-weighted problem ----------------
 * What a robust loss did to every measurement at a global X ((d+1)N x d, the layout above: t_p = row p, Y_p = R_p^T =
 * rows N + d p ..).  For edge e = (i, j, R_e, t_e, kappa_e, tau_e), in graph (file) order:
 *   s_rot_e   = kappa_e |Y_j - R_e^T Y_i|_F^2
 *   s_trans_e = tau_e |t_j - t_i - t_e^T Y_i|^2
 *   s_e       = s_rot_e + s_trans_e       (the squared norm of the edge's residual rows, DPGO_utils.cpp:1643-1677)
 * An edge is INTER when its endpoints lie in different nodes of the graph's partition.  Intra edges, and every edge under
 * loss 0 (None): rho = s, w = 1.  Inter edges (DPGOProblem.cpp:651-670, delta = loss_reg):
 *   1 Huber          w = sqrt(delta) / sqrt(max(s, delta)),   rho = min(2 sqrt(delta) sqrt(max(s, delta)) - delta, s)
 *   2 GemanMcClure   w = delta^2 / (s + delta)^2,             rho = delta s / (s + delta)
 *   3 Welsch         w = exp(-s / delta),                     rho = delta - delta w
 *   F = 1/2 sum_intra s_e + 1/2 sum_inter rho_e               (DPGOStar::evaluate_f, DPGOStar.cpp:713-761)
 * One fp64 kernel, one lane per edge; the sums are reduced in a fixed order without atomics, so a second call returns the
 * same bits.  A stand-alone handle, as PCM is: no group is needed and any partition works.  There is no CPU path. */
typedef struct dpgo_edge_summary {
  double F, F_intra, F_inter;   /* F = F_intra + F_inter */
  double weight_min;            /* the smallest weight over all edges */
  int num_inter;
  int num_downweighted;         /* edges with w < 1 */
} dpgo_edge_summary_t;
typedef struct dpgo_edge_eval dpgo_edge_eval_t;
/* uploads the graph's edge records once; -1 without a HIP device, or on a NULL argument */
int dpgo_edge_eval_create(const dpgo_graph_t *g, int device, dpgo_edge_eval_t **out);
void dpgo_edge_eval_free(dpgo_edge_eval_t *h);
/* s_rot, s_trans, rho, weight: num_edges doubles each, any of them may be NULL; sum may be NULL.  -1 on X NULL,
 * ld < (d+1)N, a loss outside 0..3, or a robust loss with loss_reg not finite and positive. */
int dpgo_edge_eval_run(dpgo_edge_eval_t *h, const double *X, int ld, int loss, double loss_reg, double *s_rot,
                       double *s_trans, double *rho, double *weight, dpgo_edge_summary_t *sum);
/* device time of the last run's kernels in milliseconds (HIP events around the two launches; tools/edge_bench.py) */
int dpgo_edge_eval_kernel_ms(const dpgo_edge_eval_t *h, double *ms);
/* Debug, host only (no GPU needed): the kernel's computation lane by lane, from the same records through the same code,
 * summed in the device's order.  The host's exp / expm1 and its unfused multiply-adds round differently, so the values agree
 * with the device's to rounding, not to the bit.  Arguments as for dpgo_edge_eval_run. */
int dpgo_debug_edge_eval_host(const dpgo_graph_t *g, const double *X, int ld, int loss, double loss_reg, double *s_rot,
                              double *s_trans, double *rho, double *weight, dpgo_edge_summary_t *sum);
/* The sibling of dpgo_graph_filter_edges: the same poses, partition, R, t and edge order, kappa_e and tau_e multiplied by
 * w[e] (num_edges weights).  w[e] = 0 is legal -- the edge stays in the pattern with zero values (Welsch reaches exactly
 * 0.0) -- a negative or non-finite weight returns -1. */
int dpgo_graph_scale_edges(const dpgo_graph_t *g, const double *w, dpgo_graph_t **out);
/* The certificate of the RE-WEIGHTED problem at X, in one call: the edge evaluation at X, dpgo_graph_scale_edges by its
 * weights w_e = w(s_e(X)), a group hosting every node of the scaled graph with dpgo_options_driver(0 (None), 1) and
 * max_iterations = 0, dpgo_group_verify on it (V0 = NULL), everything released.  S_w(X) is the certificate matrix of the
 * data matrix M_w = M_intra + sum_inter w_e M_e.
 *
 * What DPGO_CERT_PROVEN means HERE.  The gradient of the robust objective at X is M_w X (evaluate_grad,
 * DPGOStar.cpp:763-829), so `stationarity` = |S_w X|_F is the robust Riemannian gradient norm.  rho is concave in s for
 * the three losses, so the quadratic surrogate F_w(Z) + c >= F_robust(Z) for every Z, with equality at X.  S_w(X) >= -eta I
 * together with a small stationarity therefore says: X is the GLOBAL minimiser of its own surrogate F_w -- a fixed point of
 * an exact majorisation-minimisation step.  It does NOT say that X is the global minimum of the robust objective (the
 * surrogate of another point may reach lower).  With loss 0, or a partition of one node, every weight is 1 and the results
 * equal dpgo_group_verify's on the graph itself.  SKIPPED and max_factor_bytes as in dpgo_group_verify.  A second group is
 * built per call (seconds of set-up at 100 000 poses); cert_opts NULL: the defaults; edge_summary, x may be NULL. */
int dpgo_graph_verify_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                 const dpgo_cert_options_t *cert_opts, long long max_factor_bytes,
                                 dpgo_cert_result_t *cert_result, dpgo_cert_factor_t *cert_factor,
                                 dpgo_edge_summary_t *edge_summary, double *x, int ldx);

/* ---- marginal pose covariances ------------------------------------------------------------------------------------
 * How uncertain is each pose at X?  The inverse of the Riemannian Hessian of F = 1/2 tr(X^T M X) in tangent coordinates,
 * with pose `anchor` (a global pose index) held fixed: the covariance relative to the anchor, as g2o and GTSAM report
 * marginal covariances.  Unknowns dof p + a with dof = d + d (d - 1) / 2 (6 for SE(3), 3 for SE(2)): a < d the translation
 * increment t_p + dt in the world frame, then omega with R_p <- R_p Exp(hat(omega)) in the body frame (on the record:
 * Ydot_p = -hat(omega) Y_p); hat(omega) = [[0, -omega], [omega, 0]] for d = 2.  H_pq[a, b] = tr(E_a(p)^T S_pq E_b(q)) with
 * E_i = e_0 e_i^T, E_{d+k} = [0 ; -hat(e_k) Y_p] and S_pq the block of S = M - blkdiag(0, Lambda(X)) (no eta).
 *
 * The same restrictions as the certificate, for the same reasons: the TRIVIAL LOSS only (a group created with a robust
 * loss returns -1; dpgo_graph_covariance_reweighted below is the route for whoever optimised with one), and the group must
 * HOST EVERY NODE of the graph (-1 otherwise).  The optimiser's state is not touched.
 *
 * The device writes H into the value array of a multifrontal factor of its own (k_cov_hessian), factors it, and a selected
 * inversion (products on the fp64 matrix cores, top-down through the elimination tree) gives the entries of H^-1 inside the
 * factor's pattern, which holds every pose's diagonal block and the block of every edge.
 *   marginals  N x dof x dof doubles by global pose, each block row-major
 *   cross      npairs x dof x dof: Sigma_pq of the requested pairs (pairs: 2 npairs global poses).  Every pair must be an
 *              edge of the graph (or p == q): a pair that is not returns -1.  pairs, cross may be NULL with npairs = 0.
 *   Every block that involves the anchor is zero.
 *   result     outcome COV_OK; COV_NOT_PD when the anchored H is not positive definite (a saddle or a maximum; the
 *              blocks are zero); COV_SKIPPED when the analysis predicts more device bytes than max_bytes (> 0) or than half
 *              of the free device memory (the outputs are not written, nothing of the factor is allocated).  unknowns,
 *              fronts, levels, max_front, device_bytes are filled for SKIPPED too; stationarity = |S X|_F says whether X
 *              is a critical point at all; symbolic_s: host seconds of the analysis (0 after a group's first call);
 *              numeric_ms: host milliseconds from the launch of k_cov_hessian to the finished blocks on the device.
 * A local minimum has covariances even where its certificate is NEGATIVE. */
#define DPGO_COV_OK 0
#define DPGO_COV_NOT_PD 1
#define DPGO_COV_SKIPPED 2
typedef struct dpgo_cov_result {
  int outcome, unknowns, fronts, levels, max_front;
  long long device_bytes;
  double pivot_min, pivot_max, stationarity, symbolic_s, numeric_ms;
  double factor_ms, selinv_ms;   /* numeric_ms taken apart: up to the factorisation's verdict; the selected inversion */
  double selinv_flops;           /* useful flops of its products: sum over the fronts of 2 u^2 w + 2 u w^2 + w^3 */
} dpgo_cov_result_t;
int dpgo_group_covariance(dpgo_group_t *grp, const double *X, int ld, int anchor, long long max_bytes, const int *pairs,
                          int npairs, double *marginals, double *cross, dpgo_cov_result_t *result);
/* Debug: the anchored H as the device wrote it, read back from the value array of the factorisation: CSR with dof N + 1 row
 * pointers on the unknowns dof g + a of the GLOBAL poses g, every stored block dense, the anchor's row and column those of
 * the identity.  With ptr = col = val = NULL only *nnz is set; otherwise cap >= *nnz. */
int dpgo_group_cov_hessian(dpgo_group_t *grp, const double *X, int ld, int anchor, int *ptr, int *col, double *val,
                           long long cap, long long *nnz);
/* The covariances of the RE-WEIGHTED problem at X, by the recipe of dpgo_graph_verify_reweighted: the edge evaluation at X,
 * dpgo_graph_scale_edges by its weights (frozen at X), a trivial-loss group hosting every node of the scaled graph,
 * dpgo_group_covariance on it, everything released.  This is the covariance of the majorisation-minimisation SURROGATE
 * F_w at its fixed point X -- the information matrix a re-weighted least-squares solver would report -- NOT that of the
 * robust objective, whose true Hessian also has the derivative of the weights: dpgo_group_robust_covariance (below, behind the
 * Newton polish) builds that one.  edge_summary may be NULL. */
int dpgo_graph_covariance_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                     int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                                     double *cross, dpgo_cov_result_t *result, dpgo_edge_summary_t *edge_summary);

/* ---- joint covariances of arbitrary pose pairs and loop-closure gating -------------------- */
/* dpgo_group_covariance knows the cross block of an EDGE only.  Here (p, q) are any two poses: with the factor of the same
 * anchored H, the columns of H^-1 that belong to the poses asked for are solved for on the device (a block solve on the fp64
 * matrix cores, at most 64 columns per batch) and read at the rows of p and q.  No block of a selected inversion is stored,
 * so the refusal counts the numeric phase, the solve and the call's own buffers: this may run where dpgo_group_covariance
 * answers COV_SKIPPED.  Restrictions, anchor and coordinates as for dpgo_group_covariance; the optimiser is not touched.
 *   pairs       npairs x 2 global poses; p == q, a pose equal to the anchor and repeated pairs are allowed
 *   candidates  NULL, or npairs x (d^2 + d + 2) doubles: a candidate relative measurement R~ (d x d row-major), t~ (d),
 *               kappa, tau (> 0, else -1) of every pair -- what a loop-closure edge p -> q would carry
 *   joint       npairs x 3 x dof^2: Sigma_pp, Sigma_pq, Sigma_qq, row-major.  Sigma_pq has the ROWS of p and the COLUMNS of
 *               q, Sigma_pq[a][b] = cov(x_p[a], x_q[b]), as `cross` of dpgo_group_covariance.  Blocks that involve the anchor
 *               are exact zeros; a pair's bits do not depend on what else the call asks for
 *   rel         npairs x dof^2: the covariance of T_pq = T_p^-1 T_q in the same perturbation (t_pq + dt, R_pq Exp(hat(domega))),
 *               J Sigma_joint J^T with domega_pq = omega_q - R_pq^T omega_p, dt_pq = R_p^T (dt_q - dt_p) + hat(t_pq) omega_p
 *   gate        with candidates (else ignored; NULL with candidates: -1), npairs x (2 + dof): d^2 = r^T S^-1 r, not_pd (1.0
 *               where S is not positive definite, and then d^2 = 0), the residual r = [t_pq - t~ ; vee Log(R~^T R_pq)];
 *               S = rel + Omega^-1, Omega = blkdiag(tau I_d, 2 kappa I_{dof-d}).  No threshold is applied: compare d^2 with
 *               the chi-square quantile (dof degrees of freedom) of your choice
 *   result      outcome PAIRS_OK, PAIRS_NOT_PD (the anchored H is not positive definite; the outputs are zero) or
 *               PAIRS_SKIPPED (device_bytes above max_bytes (> 0) or above half of the free device memory; the outputs are
 *               not written, nothing is allocated); columns: unit columns solved (dof per distinct non-anchor pose), batches:
 *               solves; factor_ms / solve_ms / gate_ms: host milliseconds of the three phases, each ending in a synchronise */
#define DPGO_PAIRS_OK 0
#define DPGO_PAIRS_NOT_PD 1
#define DPGO_PAIRS_SKIPPED 2
typedef struct dpgo_pairs_result {
  int outcome, unknowns, fronts, levels, max_front, columns, batches, reserved;
  long long device_bytes;
  double pivot_min, pivot_max, stationarity, symbolic_s, factor_ms, solve_ms, gate_ms;
  double solve_flops;    /* useful flops of the batches: sum over the fronts of 4 (w + u) w, times every batch's columns rounded up to 16 */
  double factor_bytes;   /* factor bytes the batches stream: 16 sum (w + u) w per batch */
} dpgo_pairs_result_t;
int dpgo_group_pair_covariance(dpgo_group_t *grp, const double *X, int ld, int anchor, long long max_bytes, const int *pairs,
                               int npairs, const double *candidates, double *joint, double *rel, double *gate,
                               dpgo_pairs_result_t *result);
/* The same for the RE-WEIGHTED problem at X, by dpgo_graph_covariance_reweighted's recipe. */
int dpgo_graph_pair_covariance_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                          int anchor, long long max_bytes, const int *pairs, int npairs, const double *candidates,
                                          double *joint, double *rel, double *gate, dpgo_pairs_result_t *result,
                                          dpgo_edge_summary_t *edge_summary);
/* Measurement (tools/pair_bench.py): what there was before the block solve -- the anchored H of X written and factored as
 * above, then ncols right-hand sides solved ONE AT A TIME with the single-vector device solve on the same factor, ending in
 * a synchronise; *ms: host milliseconds of the ncols solves.  -1 where the call above would be refused or H is not positive
 * definite. */
int dpgo_debug_pairs_vsolve_baseline(dpgo_group_t *grp, const double *X, int ld, int anchor, int ncols, double *ms);
/* Debug (no device): the column plan of a call -- poses (room for 2 npairs): the distinct non-anchor poses, ascending;
 * pair_col (2 npairs): the first column of every pair's p and q, -1 for the anchor; sizes[4]: poses, columns, batches, kb. */
int dpgo_debug_pairs_plan(int dof, int anchor, const int *pairs, int npairs, int *poses, int *pair_col, int *sizes);
/* Debug (no device): the arithmetic of one pair on the host, the code k_pairs_gate runs -- recp / recq: the pose records
 * (t, then R^T row-major), joint: 3 dof^2, cand: d^2 + d + 2 doubles or NULL; rel: dof^2, gate: 2 + dof (with cand). */
int dpgo_debug_pairs_gate(int d, const double *recp, const double *recq, const double *joint, const double *cand, double *rel,
                          double *gate);

/* ---- joint marginals of a pose set: covariance and information ---------------------------- */
/* What does the graph know about a SET of poses together?  keep lists nkeep distinct global poses in any order; with the factor
 * of the same anchored H the columns of H^-1 of the kept poses are solved for (the batches of dpgo_group_pair_covariance) and
 * read at the kept rows: Sigma_KK, in the order of the LIST.  Restrictions, anchor and coordinates as for
 * dpgo_group_covariance; X should be a critical point (dpgo_group_polish); the optimiser is not touched.
 *   base < 0    the absolute form: n = dof nkeep, cov = Sigma_KK with the anchor held fixed.  The anchor may not be kept (-1):
 *               its block is exactly zero and no information form exists
 *   base >= 0   the relative form: base is one of at least two kept poses (else -1), n = dof (nkeep - 1), cov = J Sigma_KK J^T:
 *               the joint covariance of T_base^-1 T_k of the other kept poses in list order, in dpgo_group_pair_covariance's
 *               perturbation of T_pq (for nkeep = 2 this is its `rel`).  The anchor may be kept or be the base: its blocks of
 *               Sigma_KK are zeros.  To first order at a critical point this does not depend on the anchor
 *   cov         n x n row-major, symmetric bit for bit; the lower entries of the absolute form are the bits of
 *               dpgo_group_pair_covariance's joint blocks
 *   info        with want_info (else ignored): cov^-1, n x n, symmetric bit for bit -- in the absolute form the Schur complement
 *               of the anchored H onto the kept poses.  A dense factor of order n by the multifrontal kernels (one front) and
 *               its selected inverse; kept with the group per n
 *   logdet      with want_info: log det cov (the set's differential entropy up to constants); 0 otherwise
 *   result      outcome MARG_OK, MARG_NOT_PD (the anchored H is not positive definite; the outputs are zero) or MARG_SKIPPED
 *               (device_bytes above max_bytes (> 0) or above half of the free device memory; the outputs are not written,
 *               nothing is allocated); info_not_pd: the factorisation of cov met a non-positive pivot -- cov is delivered,
 *               info and logdet are zeros; n, columns, batches: filled for SKIPPED too; dense_pivot_min / max: of cov's
 *               factorisation; factor_ms / solve_ms / dense_ms: host milliseconds of the three phases */
#define DPGO_MARG_OK 0
#define DPGO_MARG_NOT_PD 1
#define DPGO_MARG_SKIPPED 2
typedef struct dpgo_marg_result {
  int outcome, unknowns, fronts, levels, max_front, info_not_pd, n, columns, batches, reserved;
  long long device_bytes;
  double pivot_min, pivot_max, dense_pivot_min, dense_pivot_max, stationarity, symbolic_s, factor_ms, solve_ms, dense_ms;
} dpgo_marg_result_t;
int dpgo_group_joint_marginal(dpgo_group_t *grp, const double *X, int ld, const int *keep, int nkeep, int anchor, int base,
                              int want_info, long long max_bytes, double *cov, double *info, double *logdet,
                              dpgo_marg_result_t *result);
/* The same for the RE-WEIGHTED problem at X, by dpgo_graph_covariance_reweighted's recipe and with its caveat. */
int dpgo_graph_joint_marginal_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                         const int *keep, int nkeep, int anchor, int base, int want_info, long long max_bytes,
                                         double *cov, double *info, double *logdet, dpgo_marg_result_t *result,
                                         dpgo_edge_summary_t *edge_summary);
/* Debug (no device): the column plan of a call -- poses (room for nkeep): the kept poses other than the anchor, in list order;
 * col (nkeep): the first column of every kept pose, -1 for the anchor; sizes[4]: poses, columns, batches, kb. */
int dpgo_debug_marg_plan(int dof, int anchor, const int *keep, int nkeep, int *poses, int *col, int *sizes);
/* Debug: the relative covariance from a GIVEN Sigma_KK ((dof nkeep)^2, list order) and the kept poses' records X (nkeep x
 * (d + 1) d: t, then R^T row-major); base_pos: the base's position in the list; cov: (dof (nkeep - 1))^2.  _host: the shared
 * arithmetic on the host (no device); the other: the kernel on the same inputs.  The two agree bit for bit. */
int dpgo_debug_marg_rel_host(int d, int nkeep, int base_pos, const double *X, const double *sigma, double *cov);
int dpgo_debug_marg_rel(int device, int d, int nkeep, int base_pos, const double *X, const double *sigma, double *cov);
/* Debug: the gather (batches of 64 columns), the dense factorisation, the inverse and the log-determinant on a GIVEN dense
 * symmetric matrix A of order n, no graph: cov <- the gathered copy of A, info <- A^-1, *logdet <- log det A; result: n,
 * columns, batches, info_not_pd (then info and logdet are zeros), the dense pivots, device_bytes of the dense factor. */
int dpgo_debug_marg_dense(int device, int n, const double *A, double *cov, double *info, double *logdet, dpgo_marg_result_t *result);

/* ---- joint compatibility and budgeted selection of loop-closure candidates ---------------- */
/* dpgo_group_pair_covariance gates ONE candidate at a time.  Here ncand candidates are judged together, in its perturbation and
 * sign conventions.  pairs[ncand][2]: global poses, p != q (-1); a pair may repeat, pairs may share poses, either end may be the
 * anchor.  candidates[ncand][d^2 + d + 2]: R~, t~, kappa, tau, both weights positive (-1).  Restrictions, anchor and coordinates
 * as for dpgo_group_covariance; X should be a critical point (dpgo_group_polish); the optimiser is not touched.
 *   K           the distinct end poses in order of first appearance (p_0, q_0, p_1, ...); n = dof ncand
 *   cov         (optional) n x n row-major: J Sigma_KK J^T, the joint covariance of the candidates' predicted relative poses;
 *               symmetric bit for bit; its diagonal blocks are dpgo_group_pair_covariance's `rel`
 *   S           (optional) n x n: cov + blkdiag(Omega_i^-1), Omega_i = blkdiag(tau_i I_d, 2 kappa_i I_{dof - d})
 *   residual    n: the stacked residuals of dpgo_group_pair_covariance's gate
 *   info        with want_joint (else ignored): S^-1 by the dense factor of dpgo_group_joint_marginal, kept with the group per n
 *   scalars[5]  logdet S, d2_joint = r^T S^-1 r, gain_all = 1/2 (logdet S - sum_i log det Omega_i^-1) (zeros without
 *               want_joint or with joint_not_pd), gain_selected, d2_selected (the sums over the chosen steps)
 *   budget      > 0: the greedy selection of at most budget candidates by conditional information gain
 *               gain_i = 1/2 (log det C_i - log det Omega_i^-1), C_i the candidate's innovation covariance given the candidates
 *               already chosen; eligible iff C_i is positive definite and (d2_max <= 0 or the CONDITIONAL d2_i <= d2_max); ties go
 *               to the lowest index.  The loop runs on the device with no host round trip between steps and stops at the first
 *               step without an eligible candidate.  gain_selected = 1/2 (log det S_sel - log det R_sel) and
 *               d2_selected = r_sel^T S_sel^-1 r_sel of the chosen principal submatrix
 *   selected    budget ints: the chosen candidates in order, -1 past n_selected
 *   steps       budget x 4: index, gain, d2, the number of eligible candidates at that step; zeros past n_selected
 *   poses       room for 2 ncand ints: K, the first result->poses entries
 *   result      outcome CAND_OK, CAND_NOT_PD (the anchored H is not positive definite; the outputs are zero) or CAND_SKIPPED
 *               (device_bytes above max_bytes (> 0) or above half of the free device memory; only poses is written, nothing is
 *               allocated); joint_not_pd: the factorisation of S met a non-positive pivot -- info and scalars[0..2] are zeros,
 *               the selection still ran; n, poses, columns, batches: filled for SKIPPED too */
#define DPGO_CAND_OK 0
#define DPGO_CAND_NOT_PD 1
#define DPGO_CAND_SKIPPED 2
typedef struct dpgo_cand_result {
  int outcome, unknowns, fronts, levels, max_front, joint_not_pd, n, poses, columns, batches, n_selected, reserved;
  long long device_bytes;
  double pivot_min, pivot_max, dense_pivot_min, dense_pivot_max, stationarity, symbolic_s, factor_ms, solve_ms, dense_ms, select_ms;
} dpgo_cand_result_t;
int dpgo_group_candidate_set(dpgo_group_t *grp, const double *X, int ld, const int *pairs, int ncand, const double *candidates,
                             int anchor, int budget, double d2_max, int want_joint, long long max_bytes, double *cov, double *S,
                             double *residual, double *info, double *scalars, int *selected, double *steps, int *poses,
                             dpgo_cand_result_t *result);
/* The same for the RE-WEIGHTED problem at X, by dpgo_graph_pair_covariance_reweighted's recipe and with its caveat. */
int dpgo_graph_candidate_set_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                        const int *pairs, int ncand, const double *candidates, int anchor, int budget, double d2_max,
                                        int want_joint, long long max_bytes, double *cov, double *S, double *residual, double *info,
                                        double *scalars, int *selected, double *steps, int *poses, dpgo_cand_result_t *result,
                                        dpgo_edge_summary_t *edge_summary);
/* Debug: the block kernel on a GIVEN Sigma_KK ((dof nposes)^2, list order), the listed poses' records X (nposes x (d + 1) d) and
 * kpos[ncand][2], the positions of every candidate's ends in the list: cov (optional), S ((dof ncand)^2), residual (dof ncand).
 * _host: the shared arithmetic on the host (no device); the other: the kernels.  cov and S agree bit for bit. */
int dpgo_debug_cand_innov_host(int d, int ncand, int nposes, const int *kpos, const double *X, const double *sigma,
                               const double *candidates, double *cov, double *S, double *residual);
int dpgo_debug_cand_innov(int device, int d, int ncand, int nposes, const int *kpos, const double *X, const double *sigma,
                          const double *candidates, double *cov, double *S, double *residual);
/* Debug: the selection on a GIVEN S ((dof ncand)^2), r and weights[ncand][2] (kappa, tau), no graph.  selected (budget) and steps
 * (budget x 4) are read AND written: only the chosen steps are written, entries from *n_selected on keep the caller's values.
 * sums[2]: gain_selected, d2_selected.  _host: the same steps on the host (no device). */
int dpgo_debug_cand_select_host(int d, int ncand, int budget, double d2_max, const double *S, const double *r, const double *weights,
                                int *selected, double *steps, double *sums, int *n_selected);
int dpgo_debug_cand_select(int device, int d, int ncand, int budget, double d2_max, const double *S, const double *r,
                           const double *weights, int *selected, double *steps, double *sums, int *n_selected);

/* ---- measurement sensitivities: implicit differentiation of the solution ------------------ */
/* How does the solution depend on the measurements it was computed from?  At a critical point X* the implicit function
 * theorem gives dX* / dtheta = -H^-1 d_theta g, with H the anchored tangent-space Hessian of dpgo_group_covariance and g the
 * tangent gradient.  For k scalars L_l(X*) whose tangent gradients at X* are the columns c_l of `upstream`, the adjoints
 * lambda_l = H^-1 c_l are solved for on the device (the factor and the block solve of dpgo_group_pair_covariance, at most 64
 * columns per batch), and one kernel gives, for EVERY edge e and every l,
 *     dL_l / dtheta_e = -d phi_e / d theta_e,    phi_e(lambda; theta_e) = D_lambda (1/2 tau |t_j - t_i - R_i t~|^2 + 1/2 kappa |R_j - R_i R~|_F^2)
 * -- the mixed second derivative of the edge's own term.  Restrictions, anchor and coordinates as for dpgo_group_covariance;
 * X should be a critical point (dpgo_group_polish): `stationarity` reports |S X|_F, nothing is enforced.  The optimiser is not
 * touched.  The robust objective has a call of its own, dpgo_group_robust_sensitivity (below, behind the Newton polish); the
 * re-weighted problem is reached through dpgo_graph_scale_edges.
 *   graph       the graph the group was created from (or one of the same poses whose every edge is a block of the group's
 *               pattern: the rule of dpgo_group_robust_polish, -1 otherwise); it fixes the order of the edges in `sens`
 *   upstream    (dof N) x k column-major, ldu >= dof N, by global pose: entry dof p + a of a column is the derivative of L along
 *               coordinate a of pose p (a < d: t_p + dt in the world frame; the rest: R_p <- R_p Exp(hat(omega))).  The anchor's
 *               rows are ignored.  A non-finite entry: -1
 *   adjoint     NULL, or (dof N) x k column-major: lambda_l by global pose, exact zeros on the anchor
 *   sens        k x num_edges x (2 + dof): [l][e][d/dkappa, d/dtau, d/dt~[0..d), d/deta[0..dof-d)], with t~ + dt~ (raw entries)
 *               and R~ <- R~ Exp(hat(eta)).  Column l's bits do not depend on k, on its position or on the other columns
 *   result      outcome SENS_OK, SENS_NOT_PD (the anchored H is not positive definite; the outputs are zero) or SENS_SKIPPED
 *               (device_bytes above max_bytes (> 0) or above half of the free device memory; the outputs are not written,
 *               nothing is allocated); columns: k, batches: block solves, edges: num_edges; factor_ms / solve_ms / edge_ms:
 *               host milliseconds of the factorisation, of the batches' uploads, solves and adjoint read-outs, and of the
 *               edge kernel with the copies of its output, each ending in a synchronise */
#define DPGO_SENS_OK 0
#define DPGO_SENS_NOT_PD 1
#define DPGO_SENS_SKIPPED 2
typedef struct dpgo_sens_result {
  int outcome, unknowns, fronts, levels, max_front, columns, batches, edges;
  long long device_bytes;
  double pivot_min, pivot_max, stationarity, symbolic_s, factor_ms, solve_ms, edge_ms;
} dpgo_sens_result_t;
int dpgo_group_sensitivity(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, long long max_bytes,
                           const double *upstream, int ldu, int k, double *adjoint, double *sens, dpgo_sens_result_t *result);
/* Debug (no device): the arithmetic of k_sens_edge on the host for one adjoint -- lambda: dof N by global pose (used as given:
 * no anchor is struck out); sens: num_edges x (2 + dof) in the order above; phi: num_edges (phi_e) or NULL. */
int dpgo_debug_sens_edge_host(const dpgo_graph_t *graph, const double *X, int ld, const double *lambda, double *sens, double *phi);

/* ---- per-edge reliability: redundancy numbers and the leave-one-out chi-square ------------ */
/* How well is each measurement of the graph checked by the others, and does it agree with them?  The gate of
 * dpgo_group_pair_covariance answers for a CANDIDATE: for an edge that is already in the graph its d^2 counts the edge twice.
 * With rel = J Sigma_joint J^T, r and Omega = blkdiag(tau I_d, 2 kappa I_{dof-d}) as there -- the edge's own (R~, t~, kappa, tau)
 * taken as the candidate -- the quantities of an existing edge are built on the residual covariance C = Omega^-1 - rel:
 *     d2_loo = r^T C^-1 r (Baarda / Pope data snooping; compare with a chi-square quantile of dof degrees of freedom; 1/2 d2_loo
 *     is the first-order drop of the optimum when the edge is removed),  r_loo = Omega^-1 C^-1 r (the residual the edge would have
 *     at the solution of the graph without it),  influence = z^T rel z with z = C^-1 r (the H-norm squared of the displacement of
 *     that solution),  redundancy = dof - sum_i Omega_ii rel_ii,  redundancy_trans = d - tau sum_{i<d} rel_ii,  d2_own = r^T Omega r.
 * No threshold is applied.  Restrictions, anchor and coordinates as for dpgo_group_covariance; X should be a critical point
 * (dpgo_group_polish); the optimiser is not touched.
 *   graph       as for dpgo_group_sensitivity (-1 otherwise); it numbers the edges
 *   method      DPGO_RELY_SELINV: the selected inversion of dpgo_group_covariance, every listed edge's three blocks gathered from
 *               it on the device; DPGO_RELY_SOLVE: the block solves of dpgo_group_pair_covariance on the distinct poses of the
 *               listed edges; DPGO_RELY_AUTO: SELINV where its bytes are not refused, otherwise SOLVE, otherwise SKIPPED
 *   edges       NULL (every edge of the graph, nedges ignored), or nedges indices into the graph's edges: any order, repeats
 *               allowed; an index outside the graph: -1
 *   records     one row per listed edge, 6 + 2 dof doubles: d2_loo, flag, redundancy, redundancy_trans, d2_own, influence, r[dof],
 *               r_loo[dof].  flag 0: C is positive definite (every pivot of its Cholesky factor positive).  1: it is not (no
 *               redundancy, or the Gauss-Newton model does not hold at X): d2_loo, influence, r_loo are exact zeros, the rest is
 *               filled.  2: kappa or tau of the edge is not > 0 (dpgo_graph_scale_edges can leave that): zeros but the flag
 *   rel, joint  NULL, or per listed edge dof^2 / 3 dof^2 doubles as dpgo_group_pair_covariance hands them out
 *   result      outcome RELY_OK, RELY_NOT_PD (the anchored H is not positive definite; the outputs are zero) or RELY_SKIPPED (the
 *               bytes of the method above max_bytes (> 0) or above half of the free device memory; the outputs are not written,
 *               nothing is allocated); device_bytes_selinv / device_bytes_solve: what either method would allocate, filled for
 *               SKIPPED too, device_bytes: of method_used; edges: listed, flagged: flag 1, unweighted: flag 2; redundancy_sum:
 *               the records' redundancy summed in list order, flag-2 edges left out (dof (m - N + 1) over a whole graph with
 *               zero residuals); columns / batches: of the SOLVE plan; factor_ms / inverse_ms / edge_ms: host milliseconds of
 *               the factorisation, of the inversion and the gather (or the batches), and of the two edge kernels with the
 *               copies of their output, each ending in a synchronise */
#define DPGO_RELY_OK 0
#define DPGO_RELY_NOT_PD 1
#define DPGO_RELY_SKIPPED 2
#define DPGO_RELY_AUTO 0
#define DPGO_RELY_SELINV 1
#define DPGO_RELY_SOLVE 2
typedef struct dpgo_rely_result {
  int outcome, method_used, unknowns, fronts, levels, max_front, edges, flagged, unweighted, columns, batches, reserved;
  long long device_bytes, device_bytes_selinv, device_bytes_solve;
  double redundancy_sum, pivot_min, pivot_max, stationarity, symbolic_s, factor_ms, inverse_ms, edge_ms;
} dpgo_rely_result_t;
int dpgo_group_edge_reliability(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, long long max_bytes,
                                int method, const int *edges, int nedges, double *records, double *rel, double *joint,
                                dpgo_rely_result_t *result);
/* The same for the RE-WEIGHTED problem at X, by dpgo_graph_covariance_reweighted's recipe: the loss weights frozen at X, a
 * trivial-loss group of the scaled graph.  It describes the MM surrogate, not the robust objective.  edge_summary may be NULL. */
int dpgo_graph_edge_reliability_reweighted(const dpgo_graph_t *g, int device, const double *X, int ld, int loss, double loss_reg,
                                           int anchor, long long max_bytes, int method, const int *edges, int nedges, double *records,
                                           double *rel, double *joint, dpgo_rely_result_t *result, dpgo_edge_summary_t *edge_summary);
/* Debug (no device): the arithmetic of one record on the host, the code k_rely_edge runs, for n edges -- rel: n x dof^2, r: n x dof,
 * kappa, tau: n each; records: n x (6 + 2 dof). */
int dpgo_debug_rely_edge_host(int d, int n, const double *rel, const double *r, const double *kappa, const double *tau,
                              double *records);
/* Debug: k_rely_edge alone on the same arrays (host pointers), on HIP device `device`. */
int dpgo_debug_rely_edge(int device, int d, int n, const double *rel, const double *r, const double *kappa, const double *tau,
                         double *records);

/* ---- Newton polish: from the point the optimiser stopped at to a critical point ----------- */
/* AMM-PGO# is a first-order method; the certificate and the covariances above mean something only at a critical point.
 * dpgo_group_polish takes damped Riemannian Newton steps from X -- Levenberg-Marquardt on the anchored tangent-space Hessian
 * H of dpgo_group_covariance, written, factored and solved on the device -- until the tangent gradient g is at rounding
 * level or the step budget is spent:
 *     mu = 0;  for k = 0 ... max_steps:
 *         g, |g|, F0, H, hmax at X                      (hmax: the largest diagonal entry of H over the non-anchor unknowns)
 *         |g| <= (grad_tol > 0 ? grad_tol : rel_tol hmax) -> CONVERGED;   k == max_steps -> MAX_STEPS
 *         at most max_tries times:  factor H + mu I;  not positive definite: indefinite += 1 if mu == 0,
 *                                   mu = max(10 mu, 1e-3 hmax), next try
 *             delta = -(H + mu I)^-1 g;  Z = retract(X, delta);  F1 = F(Z)
 *             pred = -1/2 g'delta + 1/2 mu |delta|^2;  rho = pred > 0 ? (F0 - F1) / pred : -1
 *             accept if rho >= 0.1 or |F0 - F1| <= 1e-13 |F0|:  X = Z;  rho > 0.75: mu /= 10, and mu = 0 once mu < 1e-8 hmax
 *             else mu = max(10 mu, 1e-3 hmax)
 *         no try accepted -> STALLED (the last accepted point is returned)
 * retract: t_p + dt, R_p Exp(hat(omega)) in the coordinates of dpgo_group_covariance.  F never increases except through the
 * rounding clause.  The same restrictions as the covariance: the TRIVIAL LOSS only, the group must HOST EVERY NODE, the global
 * pose opt->anchor is held fixed (its rows of Xout are those of X bit for bit); -1 otherwise.  The optimiser's state is not touched.
 *   opt     NULL: the defaults
 *   Xout    (d+1) N x d column-major, ldout >= (d+1) N: the new point (not written for SKIPPED); may be X itself
 *   log     optional, log_cap rows of 5 doubles: per iteration k its F0, |g|, mu at entry, rho of the accepted try, tries
 *   result  outcome; steps (accepted), factorisations, indefinite (factorisations at mu = 0 that met a non-positive pivot:
 *           the starting region was not convex); F and |g| at the first and the last point, hmax and mu at the end, the pivot
 *           range of the last factor; unknowns, fronts, levels, max_front, device_bytes from the symbolic analysis (filled for
 *           SKIPPED too); symbolic_s: host seconds of the analysis (0 after a group's first covariance or polish call);
 *           total_ms and its parts: factor_ms (the Hessian from its launch to the read-back behind it, and the
 *           factorisations up to their verdicts), solve_ms (the vector
 *           solves with the retraction and F(Z) behind them), other_ms.
 * SKIPPED when what polish allocates -- the numeric phase, the vector solve, three vectors; not the blocks of the selected
 * inversion -- is more than max_bytes (> 0), or what of it is still to be allocated is more than half of the free device
 * memory: nothing is allocated then. */
#define DPGO_POLISH_CONVERGED 0
#define DPGO_POLISH_MAX_STEPS 1
#define DPGO_POLISH_STALLED 2
#define DPGO_POLISH_SKIPPED 3
typedef struct dpgo_polish_options {
  int max_steps, max_tries;   /* 20, 8 */
  double rel_tol, grad_tol;   /* 1e-9, 0 */
  int anchor;                 /* 0: the global pose held fixed */
} dpgo_polish_options_t;
typedef struct dpgo_polish_result {
  int outcome, steps, factorisations, indefinite;
  double F_initial, F_final, grad_initial, grad_final, hmax, mu_final, pivot_min, pivot_max;
  int unknowns, fronts, levels, max_front;
  long long device_bytes;
  double symbolic_s, total_ms, factor_ms, solve_ms, other_ms;
} dpgo_polish_result_t;
void dpgo_polish_options_default(dpgo_polish_options_t *opt);
int dpgo_group_polish(dpgo_group_t *grp, const double *X, int ld, const dpgo_polish_options_t *opt, long long max_bytes,
                      double *Xout, int ldout, double *log, int log_cap, dpgo_polish_result_t *result);

/* ---- Hessian modes: the weakest eigenpairs of the anchored Hessian -------------------------- */
/* Which global directions does the graph determine worst, and -- where H is not positive definite -- how negative is the
 * curvature, along which poses, and which way is down?  The k smallest eigenpairs (lambda_j, v_j) of the anchored
 * tangent-space Hessian H of dpgo_group_covariance (the anchor's identity block excluded: every v_j is zero on its rows), by
 * shift-invert block subspace iteration with Rayleigh-Ritz on the covariance's factor: A = H + mu I is factored with mu = 0
 * (or opts->shift), on a non-positive pivot with mu = max(10 mu, 1e-3 hmax) at most max_tries times; a block of
 * b = 16 ceil((k + guard) / 16) <= 64 columns is solved in one batch of the block solve per iteration, the Ritz pairs of A on
 * A^-1 V come from two b x b Gram matrices, and lambda_j = theta_j - mu.  At a polished minimum 1 / values[0] is the largest
 * eigenvalue of the covariance.  An indefinite H is an input here, not a refusal.  Restrictions, anchor and coordinates as for
 * dpgo_group_covariance; the optimiser is not touched.
 *   k           1 ... 60 and at most n - dof, n = dof N (-1 otherwise)
 *   values      k: lambda_j ascending;  residuals  k: |H v_j - lambda_j v_j| from the iteration's own recurrence
 *   vectors     k x n row-major: row j the unit vector v_j, pose-major by global pose
 *   energy      k x N: |v_j|^2 restricted to pose p -- where the mode lives; every row sums to 1
 *   X_escape    with want_escape (else ignored, may be NULL): (d+1)N x d, leading dimension ld.  Where lambda_0 < 0: with g the
 *               tangent gradient, s = -sign(g'v_0) (+1 at zero), alpha_0 = 0.5 / |v_0|_inf and
 *               pred(alpha) = alpha |g'v_0| + 1/2 alpha^2 |lambda_0|, alpha is halved up to 30 times until
 *               F(retract(X, alpha s v_0)) <= F(X) - 0.1 pred(alpha): that point, result->F_escape and escape_alpha, escaped = 1;
 *               otherwise X itself and escaped = 0
 *   result      outcome CONVERGED (every |R_j| <= rel_tol hmax, j < k), MAX_ITERS (the pairs and residuals of the last
 *               iteration are delivered), STALLED (no shift made H + mu I positive definite within max_tries, or fewer than k
 *               columns of the block stayed independent) or SKIPPED (device_bytes -- the numeric phase, one batch of the block
 *               solve, the two blocks, the partial sums and polish's three vectors -- above max_bytes (> 0), or what is still
 *               to allocate above half of the free device memory: nothing is allocated, the predictions are filled);
 *               negative: converged lambda_j < 0; shift_tries: factorisations that met a non-positive pivot */
#define DPGO_MODES_CONVERGED 0
#define DPGO_MODES_MAX_ITERS 1
#define DPGO_MODES_STALLED 2
#define DPGO_MODES_SKIPPED 3
typedef struct dpgo_modes_options {
  int guard, max_iters, max_tries, want_escape;   /* 4 (at least 4), 100, 8, 0 */
  double rel_tol, shift;                          /* 1e-8, 0 */
  unsigned long long seed;                        /* 1: of the start block */
} dpgo_modes_options_t;
typedef struct dpgo_modes_result {
  int outcome, iterations, factorisations, shift_tries, block, negative, escaped, reserved;
  int unknowns, fronts, levels, max_front;
  long long device_bytes;
  double mu, hmax, stationarity, escape_alpha, F, F_escape, pivot_min, pivot_max, symbolic_s;
  double factor_ms, solve_ms, gram_ms, ritz_ms, update_ms, total_ms;
} dpgo_modes_result_t;
void dpgo_modes_options_default(dpgo_modes_options_t *opt);
int dpgo_group_hessian_modes(dpgo_group_t *grp, const double *X, int ld, int anchor, int k, const dpgo_modes_options_t *opts,
                             long long max_bytes, double *values, double *residuals, double *vectors, double *energy,
                             double *X_escape, dpgo_modes_result_t *result);
/* Debug: the kernels of the iteration on the caller's arrays, no graph.  V, W: n x b row-major with row length ld >= b,
 * b in {16, 32, 48, 64}; the columns b ... ld are neither read nor written.  anchor_row0 / dof: the anchor's rows
 * anchor_row0 ... anchor_row0 + dof (anchor_row0 < 0: none).
 *   init    V <- the start block: entry (i, j) a pure function of (seed, i, j), in (-1, 1); zeros on the anchor's rows
 *   gram    G, T (b x b row-major, symmetric bit for bit): W'W and the mirrored lower triangle of W'V
 *   update  V <- W C in place (C b x b row-major, theta b), zeros on the anchor's rows; rr, vv (b each): the column sums of
 *           (V_old C - (W C) diag(theta))^2 and of (W C)^2
 *   ritz    (_host: no device) T c = theta G c on the lower triangles: theta (b) ascending on the first *used entries, C (b x b)
 *           with C'GC = I on those columns; a pivot of the scaled G below 1e-12 drops the trailing columns */
int dpgo_debug_modes_init(int device, long long n, int b, int ld, int anchor_row0, int dof, unsigned long long seed, double *V);
int dpgo_debug_modes_gram(int device, long long n, int b, int ld, const double *W, const double *V, double *G, double *T);
int dpgo_debug_modes_update(int device, long long n, int b, int ld, int anchor_row0, int dof, const double *W, double *V,
                            const double *C, const double *theta, double *rr, double *vv);
int dpgo_debug_modes_ritz_host(int b, const double *G, const double *T, double *theta, double *C, int *used);
int dpgo_debug_modes_ritz(int device, long long n, int b, int ld, const double *W, const double *V, double *theta, double *C,
                          int *used);   /* the Gram matrices of W, V on the device, then the host's eigenproblem */

/* ---- the robust objective: a Newton polish and covariances on its TRUE Hessian ---------------- */
/* dpgo_group_polish and dpgo_group_covariance serve F = 1/2 tr(X^T M X).  Whoever optimised with a robust loss wants a critical
 * point of   F(X) = 1/2 sum_intra s_e + 1/2 sum_inter rho(s_e)   (s_e, rho, the inter rule and delta = loss_reg as in
 * dpgo_edge_eval_run) and the covariance its Hessian gives.  With w_e = rho'(s_e), c_e = 2 rho''(s_e) (Huber: 0 for s <= delta,
 * -w / s above; Geman-McClure: -4 w / (s + delta); Welsch: -2 w / delta; 0 on intra edges, under loss 0 and where w_e == 0),
 * M_e the data matrix of edge e (s_e = tr(X^T M_e X)) and g_e[dof p + a] = tr(E_a(p)^T (M_e X)_p) in the coordinates of
 * dpgo_group_covariance:
 *     M_w = sum_e w_e M_e,   g = sum_e w_e g_e,   H = H(S_w) + sum_inter c_e g_e g_e^T,   S_w = M_w - blkdiag(0, Lambda_w(X))
 * where H(.) is the matrix of dpgo_group_covariance.  curvature = 1: this H; curvature = 0: without the rank-one terms -- the
 * Hessian of the re-weighted problem, an IRLS-Newton step that converges linearly where curvature 1 converges quadratically.
 * Everything is written on the device (robust.h: four fp64 kernels, fixed-order sums, the same bits run to run) into the
 * covariance's factor: pattern, analysis and numeric context are shared with dpgo_group_polish / dpgo_group_covariance.
 *
 * grp is a TRIVIAL-LOSS group that HOSTS EVERY NODE of `graph`, as for every call above (-1 otherwise): the loss is an argument
 * here.  graph must have the group's d and pose count and every edge must be a block of the group's pattern (-1 otherwise) --
 * the graph the group was created from, as a rule.  -1 also on a loss outside 0..3, loss_reg not finite and positive under a
 * robust loss, or a curvature outside {0, 1}.  The optimiser's state is not touched.
 *
 * dpgo_group_robust_polish: the loop, options, outcomes, log and timers of dpgo_group_polish with the robust F, M_w X and H;
 *   F_initial / F_final are the robust F; edge_summary (optional) describes the final point.  SKIPPED by dpgo_group_polish's
 *   rule with the per-edge arrays, M_w and the lists counted in; decided before anything is allocated.
 * dpgo_group_robust_covariance: dpgo_group_covariance's factorisation, selected inversion and read-out on the robust H;
 *   stationarity = |S_w X|_F (not computed for SKIPPED).  COV_NOT_PD is a legitimate answer where the negative curvature of the
 *   loss wins.
 * dpgo_group_robust_hessian (debug): the anchored H as dpgo_group_cov_hessian hands it out; optionally grad (dof N, by global
 *   pose, zeros on the anchor), F, and per edge w, c, s_rot, s_trans and rho (num_edges each; every value of
 *   dpgo_edge_eval_run's bit for bit).
 * dpgo_group_robust_matrix (debug): M_w as dpgo_group_cert_matrix hands out S.
 * dpgo_group_robust_sensitivity: dpgo_group_sensitivity at a critical point of the robust objective, the loss threshold delta =
 *   loss_reg one more parameter.  The adjoints are lambda_l = H^-1 c_l on the TRUE robust Hessian (curvature 1), and with
 *   phi_e = D_lambda (1/2 s_e):  dL/dtheta_e = -[w_e d phi_e/d theta_e + (c_e / 2) phi_e d s_e/d theta_e],
 *   dL/ddelta = -sum_inter (d w_e/d delta) phi_e.  upstream, adjoint, anchor, max_bytes and result as for
 *   dpgo_group_sensitivity (stationarity = |S_w X|_F, not computed for SKIPPED; device_bytes counts the robust buffers too);
 *   sens: k x num_edges x (3 + dof), [l][e][d/dkappa, d/dtau, d/dt~, d/deta, the edge's term of d/ddelta]; dloss_reg: k doubles,
 *   dL_l/ddelta -- the last entries summed over the edges in ascending order.  Intra edges carry dpgo_group_sensitivity's
 *   values; an edge whose weight is exactly 0 gives exact zeros; loss 0 gives dpgo_group_sensitivity's values and zero delta
 *   terms.  SENS_NOT_PD is a legitimate answer under Geman-McClure and Welsch.
 * dpgo_debug_robust_sens_edge_host (no GPU): the kernels' arithmetic for one adjoint lambda (dof N by global pose, used as
 *   given); sens: num_edges x (3 + dof), phi: num_edges or NULL.
 * dpgo_debug_robust_edge_host (no GPU): per edge w, c, rows (2 pose records: (M_e X)_i, (M_e X)_j, each t-row then d rows) and
 *   ghat (2 dof: g_e at i, at j) through the kernels' own arithmetic; any output may be NULL. */
int dpgo_group_robust_polish(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                             int curvature, const dpgo_polish_options_t *opt, long long max_bytes, double *Xout, int ldout,
                             double *log, int log_cap, dpgo_polish_result_t *result, dpgo_edge_summary_t *edge_summary);
int dpgo_group_robust_covariance(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                                 int curvature, int anchor, long long max_bytes, const int *pairs, int npairs, double *marginals,
                                 double *cross, dpgo_cov_result_t *result);
int dpgo_group_robust_sensitivity(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                                  int anchor, long long max_bytes, const double *upstream, int ldu, int k, double *adjoint,
                                  double *sens, double *dloss_reg, dpgo_sens_result_t *result);
int dpgo_debug_robust_sens_edge_host(const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                                     const double *lambda, double *sens, double *phi);
int dpgo_group_robust_hessian(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                              int curvature, int anchor, int *ptr, int *col, double *val, long long cap, long long *nnz,
                              double *grad, double *F, double *w, double *c, double *s_rot, double *s_trans, double *rho);
int dpgo_group_robust_matrix(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg,
                             int *ptr, int *col, double *val, long long cap, long long *nnz);
int dpgo_debug_robust_edge_host(const dpgo_graph_t *graph, const double *X, int ld, int loss, double loss_reg, double *w, double *c,
                                double *rows, double *ghat);

/* ---- maximum-likelihood refinement on the full information matrices, with its covariances ---- */
/* Everything above lives in the isotropic chordal model: the loader reduces every Omega_e to kappa_e, tau_e.  g2o, GTSAM and
 * Ceres minimise 1/2 sum r' Omega r with the file's Omega and hand out (J' Omega J)^-1.  For an edge e = (i -> j) with measurement
 * (R~, t~) and information Omega_e (dpgo_graph_edge_information):
 *     r_t = R~^T (R_i^T (t_j - t_i) - t~),   r_R = Log(R~^T R_i^T R_j)   (rotation vector; d = 2: the angle in (-pi, pi])
 *     F_ml(X) = 1/2 sum_e r_e' Omega_e r_e,   chi2_e = r_e' Omega_e r_e
 * in the unknowns and with the anchor convention of dpgo_group_covariance.  The gradient uses the exact Jacobians of r; the
 * Hessian is the GAUSS-NEWTON one, H = sum_e J_e' Omega_e J_e -- the Fisher information; the second-order term is left out on
 * purpose.  H is positive semidefinite by construction: NOT_PD means a rank-deficient graph.  The usual recipe is a solve in the
 * isotropic model (the optimiser, dpgo_group_polish), then this refinement from its point.
 *
 * The group is a TRIVIAL-LOSS group that HOSTS EVERY NODE, graph a graph of its poses whose every edge is a block of its
 * pattern, the anchor a pose of it, every Omega_e symmetric positive definite (checked on the host, the edge named): -1
 * otherwise.  The optimiser's state is not touched.  Edges whose rotation residual is within 1e-3 of pi are counted (near_pi);
 * their values are not specified further.
 *
 * dpgo_group_ml_polish: the loop, options, outcomes, log and timers of dpgo_group_polish with F_ml, its gradient and H;
 *   result->polish: as dpgo_group_polish fills it, the F fields F_ml; chi2_initial / chi2_final = 2 F_ml at both ends; near_pi
 *   at the final point.  SKIPPED by dpgo_group_polish's rule with the arrays of the edge pass counted in.
 * dpgo_group_ml_covariance: dpgo_group_covariance's factorisation, selected inversion, formats and outcomes on H;
 *   result->stationarity is the norm of the tangent gradient of F_ml.
 * dpgo_group_ml_hessian (debug): the anchored H as dpgo_group_cov_hessian hands it out; optionally grad (dof N, by global
 *   pose, zeros on the anchor) and F.
 * dpgo_group_ml_eval: F_ml, near_pi and per edge r (num_edges x dof) and chi2 (num_edges); for the tests also what else the
 *   edge pass left on the device: wr = Omega r (dof), grad (2 dof: the edge's gradient terms of i, of j), jw (4 dof^2:
 *   J_i, J_j, Omega J_i, Omega J_j, each row-major); any output may be NULL.
 * dpgo_debug_ml_edge_host (no GPU): the kernels' arithmetic per edge in graph order: r, wr = Omega r (dof), chi2, Ji, Jj
 *   (dof^2 row-major: rows r, columns the pose's unknowns), grad (2 dof: J_i' Omega r, J_j' Omega r), blocks (4 dof^2: the edge's
 *   terms of (i, i), (i, j), (j, i), (j, j)); any output may be NULL. */
typedef struct dpgo_ml_result {
  dpgo_polish_result_t polish;
  long long near_pi;
  double chi2_initial, chi2_final;
} dpgo_ml_result_t;
int dpgo_group_ml_polish(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, const dpgo_polish_options_t *opt,
                         long long max_bytes, double *Xout, int ldout, double *log, int log_cap, dpgo_ml_result_t *result);
int dpgo_group_ml_covariance(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, long long max_bytes,
                             const int *pairs, int npairs, double *marginals, double *cross, dpgo_cov_result_t *result);
int dpgo_group_ml_hessian(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, int *ptr, int *col,
                          double *val, long long cap, long long *nnz, double *grad, double *F);
int dpgo_group_ml_eval(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, double *F, long long *near_pi,
                       double *r, double *chi2, double *wr, double *grad, double *jw);
/* debug: k_ml_hessian on an array of the call's own -- pad doubles of `sentinel`, the nnz values (sentinels before the launch),
 * pad more -- instead of the factorisation's.  guards: the 2 pad doubles around the values as the device left them; val (cap >=
 * nnz of dpgo_group_ml_hessian): the values in that call's order. */
int dpgo_group_debug_ml_hessian_guarded(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, int pad,
                                        double sentinel, double *guards, double *val, long long cap);
int dpgo_debug_ml_edge_host(const dpgo_graph_t *graph, const double *X, int ld, double *r, double *wr, double *chi2, double *Ji,
                            double *Jj, double *grad, double *blocks, long long *near_pi);

/* ---- edge reliability and candidate gating on the full information matrices ---- */
/* dpgo_group_edge_reliability's and the gate of dpgo_group_pair_covariance's questions asked of F_ml: H = sum J' Omega J with
 * the graph's Omega, rel = J Sigma_joint J' with the exact Jacobians of the ML residual, and the statistics measured in Omega --
 * d2_loo = r' (Omega^-1 - rel)^-1 r for an edge of the graph, d2 = r' (rel + Omega^-1)^-1 r for a candidate -- evaluated in a
 * whitened form that never inverts Omega.  Both are chi-square quantities of dof degrees of freedom for anisotropic and
 * translation-rotation coupled noise.  The restrictions and the refusals are dpgo_group_ml_covariance's; stationarity is the norm
 * of the tangent gradient of F_ml; SKIPPED allocates nothing and leaves the stationarity 0.
 *
 * dpgo_group_ml_edge_reliability: the arguments, list semantics (any order, repeats allowed; NULL: every edge), methods, records
 *   (6 + 2 dof doubles; flag 2 does not occur), rel, joint and result of dpgo_group_edge_reliability.  The redundancies of all
 *   edges sum to dof (m - N + 1) at any point.
 * dpgo_group_ml_pair_gate: npairs candidates (p -> q) -- p == q and the anchor allowed -- with measurement cand_R (npairs x d^2,
 *   row-major), cand_t (npairs x d) and information cand_info (npairs x dof^2, symmetric positive definite: -1 otherwise, the
 *   candidate named).  joint, rel as dpgo_group_pair_covariance; gate: npairs x (2 + dof): d2, not_pd, the ML residual.  A
 *   candidate that copies an edge of the graph has that edge's residual bit for bit.
 * dpgo_debug_ml_rely_edge_host (no device) / dpgo_debug_ml_rely_edge: the arithmetic alone for n edges -- J: n x 2 dof^2
 *   ([J_p | J_q], each dof x dof row-major), joint: n x 3 dof^2, omega: n x dof^2, r: n x dof, sign -1 (reliability records,
 *   n x (6 + 2 dof)) or +1 (gate records, n x (2 + dof)); rel: n x dof^2.  -1: bad sizes or an omega that is not positive definite. */
int dpgo_group_ml_edge_reliability(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor,
                                   long long max_bytes, int method, const int *edges, int nedges, double *records, double *rel,
                                   double *joint, dpgo_rely_result_t *result);
int dpgo_group_ml_pair_gate(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor, long long max_bytes,
                            const int *pairs, int npairs, const double *cand_R, const double *cand_t, const double *cand_info,
                            double *joint, double *rel, double *gate, dpgo_pairs_result_t *result);
int dpgo_debug_ml_rely_edge_host(int d, int n, int sign, const double *J, const double *joint, const double *omega, const double *r,
                                 double *rel, double *records);
int dpgo_debug_ml_rely_edge(int device, int d, int n, int sign, const double *J, const double *joint, const double *omega,
                            const double *r, double *rel, double *records);

/* ---- graduated non-convexity: which measurements are outliers, and the solution without them ---- */
/* GNC-TLS and GNC-GM (Yang, Antonante, Tzoumas, Carlone, RA-L 2020) on the device.  s_e = s_rot + s_trans as dpgo_edge_eval_run
 * returns them; barc2 > 0 is the inlier threshold on s_e; the robust set R is the edges the loss may touch -- the inter-node
 * edges (robust_set NULL), or those with robust_set[e] != 0 (num_edges ints, graph order).  Edges outside R keep w_e = 1.
 *     F_w(X) = 1/2 sum_e w_e s_e,      F_mu(X) = 1/2 sum_{not R} s_e + 1/2 sum_R rho_mu(s_e)
 *     TLS:  s <= mu/(mu+1) barc2: w = 1, rho = s;   s >= (mu+1)/mu barc2: w = 0, rho = barc2;   otherwise
 *           w = sqrt(barc2 mu (mu+1) / s) - mu,   rho = 2 sqrt(barc2 mu (mu+1) s) - mu (barc2 + s)
 *     GM:   delta = mu barc2:  w = delta^2 / (s + delta)^2,   rho = delta s / (s + delta)
 *     level 0:  w = 1;  X0 = inner(X, w);  s_max = max_R s_e(X0);   R empty -> ALL_INLIERS
 *     TLS:  2 s_max <= barc2 -> ALL_INLIERS (X0, w = 1);  mu = barc2 / (2 s_max - barc2)        GM:  mu = max(1, 2 s_max / barc2)
 *     for k = 1 .. max_levels:
 *         w_R = weight_mu(s(X_{k-1}));  X_k = inner(X_{k-1}, w);   an inner STALLED -> INNER_FAILED (X_{k-1} and its weights returned)
 *         TLS:  no weight strictly between 0 and 1 -> CONVERGED;  mu = mu_step mu
 *         GM:   mu == 1 -> CONVERGED;                              mu = max(mu / mu_step, 1)
 *     k == max_levels without the above -> MAX_LEVELS
 * inner is the loop of dpgo_group_polish on the weighted problem (weights fixed, options opt->inner with its anchor).  Within a
 * level F_mu never increases.  A level whose zero weights disconnect the graph makes the Hessian singular; the shift of the
 * inner loop either copes or stalls, and a stall is INNER_FAILED, an outcome, not an error.
 * The restrictions of dpgo_group_robust_polish (a TRIVIAL-LOSS group that HOSTS EVERY NODE, every edge of graph a block of the
 * group's pattern); -1 also for a kind outside {0, 1}, barc2 not finite and positive, mu_step <= 1, max_levels < 1, bad sizes.
 * The optimiser's state is not touched.
 *   Xout     (d+1) N x d column-major, ldout >= (d+1) N (not written for SKIPPED); weights: num_edges (likewise)
 *   log      optional, log_cap rows of 10 doubles, one per level k >= 1: mu, F_mu(X_{k-1}), F_w(X_{k-1}), F_w(X_k), F_mu(X_k),
 *            inner steps, inner outcome, and the counts of w == 0, w == 1, 0 < w < 1 over R
 *   result   outcome; levels; steps and factorisations of all inner solves; the last inner outcome; mu at the first and the last
 *            level; s_max_initial (at X0); F_initial (unit weights at X); F_w and F_mu of the last level at the final point;
 *            num_robust = |R| and the three counts of the final weights; num_outliers: e in R with s_e > barc2 at the final
 *            point; device_bytes and symbolic_s as dpgo_group_polish (filled for SKIPPED too); total_ms, edge_ms (the edge
 *            passes with their read-backs), inner_ms (the inner solves).
 * SKIPPED by dpgo_group_robust_polish's rule with the arrays of the edge pass counted in; decided before anything is allocated.
 * dpgo_group_gnc_eval (debug): one edge pass at X.  w_in NULL: WEIGH -- the array starts as the caller's w, weight_mu(s_e) is
 *   written on R; otherwise FIXED: the array is w_in, read on R.  s_rot, s_trans, w (the array behind the pass): num_edges each;
 *   sums: sum_{not R} s, sum_R w s, sum_R rho_mu(s), max_R s (0 over an empty R), min_R w (+inf likewise), and the three counts.
 * dpgo_debug_gnc_weight_host (no GPU): w and rho of n values s >= 0 through the kernel's own arithmetic. */
#define DPGO_GNC_TLS 0
#define DPGO_GNC_GM 1
#define DPGO_GNC_CONVERGED 0
#define DPGO_GNC_ALL_INLIERS 1
#define DPGO_GNC_MAX_LEVELS 2
#define DPGO_GNC_INNER_FAILED 3
#define DPGO_GNC_SKIPPED 4
typedef struct dpgo_gnc_options {
  int kind;                      /* DPGO_GNC_TLS */
  double barc2, mu_step;         /* 1, 1.4 */
  int max_levels;                /* 100 */
  dpgo_polish_options_t inner;   /* dpgo_polish_options_default */
} dpgo_gnc_options_t;
typedef struct dpgo_gnc_result {
  int outcome, levels, steps, factorisations, inner_outcome;
  double mu_initial, mu_final, s_max_initial, F_initial, F_weighted_final, F_surrogate_final;
  int num_robust, num_zero, num_one, num_between, num_outliers;
  long long device_bytes;
  double symbolic_s, total_ms, edge_ms, inner_ms;
} dpgo_gnc_result_t;
void dpgo_gnc_options_default(dpgo_gnc_options_t *opt);
int dpgo_group_gnc(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, const dpgo_gnc_options_t *opt,
                   const int *robust_set, long long max_bytes, double *Xout, int ldout, double *weights, double *log, int log_cap,
                   dpgo_gnc_result_t *result);
int dpgo_group_gnc_eval(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int kind, double mu, double barc2,
                        const int *robust_set, const double *w_in, double *s_rot, double *s_trans, double *w, double *sums);
int dpgo_debug_gnc_weight_host(int kind, double mu, double barc2, const double *s, int n, double *w, double *rho);

/* ---- graduated non-convexity on the full information matrices: outlier rejection on chi2 ---- */
/* dpgo_group_gnc thresholds the isotropic s_e and ignores Omega_e.  Here GNC-TLS and GNC-GM run on the maximum-likelihood
 * objective of dpgo_group_ml_polish, with r_e, Omega_e, the unknowns, the anchor and near_pi as defined there:
 *     s_e := chi2_e = r_e' Omega_e r_e,   barc2 > 0 the caller's threshold on chi2_e -- a chi2_dof quantile, dof = 3 (d = 2) or
 *     6 (d = 3): 16.266 / 22.458 at 0.999.  (The library has no quantile function.)
 *     F_w(X) = 1/2 sum_e w_e chi2_e,   F_mu(X) = 1/2 sum_{not R} chi2_e + 1/2 sum_R rho_mu(chi2_e)
 *     g_w = sum_e w_e J_e' Omega_e r_e,   H_w = sum_e w_e J_e' Omega_e J_e   (Gauss-Newton)
 * The robust set R, the weight and rho_mu, the levels, mu's schedule, the outcomes, the options, the log's ten columns and the
 * timers are dpgo_group_gnc's, with chi2 for s; within a level F_mu never increases.  inner is the loop of dpgo_group_ml_polish
 * on (F_w, g_w, H_w) with fixed weights.  Two differences:
 *   1. An inner MAX_STEPS is normal and NOT a failure: H_w is Gauss-Newton, and at the early levels, where the weighted
 *      residuals at the minimum are large, the inner loop converges linearly.  Only an inner STALLED is INNER_FAILED.
 *   2. An edge whose weight is exactly 0 contributes exact zeros to g_w, H_w and F_w by selection, not by multiplication: an
 *      outlier's rotation residual may sit within 1e-3 of pi, where the edge's values are not specified further.  near_pi
 *      counts the edges with w_e > 0 at the final point, near_pi_all every edge.
 * The restrictions of dpgo_group_ml_polish and the argument checks of dpgo_group_gnc: -1 otherwise.  SKIPPED by
 * dpgo_group_ml_polish's rule with the weights, the robust set and the partial sums counted in; decided before anything is
 * allocated.  The optimiser's state is not touched.
 *   result->gnc   as dpgo_group_gnc fills it: s_max_initial = max_R chi2 at X0, num_outliers = e in R with chi2_e > barc2 at the
 *                 final point, the F fields on chi2
 * dpgo_group_ml_gnc_eval (debug): one edge pass at X.  w_in NULL: WEIGH -- the array starts as the caller's w, weight_mu(chi2_e)
 *   is written on R; otherwise FIXED: the array is w_in, read on R.  chi2 (unweighted), w (the array behind the pass):
 *   num_edges each; sums (10): sum_{not R} chi2, sum_R w chi2, sum_R rho_mu(chi2), max_R chi2 (0 over an empty R), min_R w
 *   (+inf likewise), the counts of w == 0, w == 1, 0 < w < 1 over R, near_pi over w > 0, near_pi over every edge.  full != 0:
 *   also r (dof), wr = w Omega r (dof), grad (2 dof: the edge's weighted gradient terms of i, of j) and jw (4 dof^2: J_i, J_j,
 *   w Omega J_i, w Omega J_j; all zeros where w == 0), each optional.
 * dpgo_group_debug_ml_gnc_hessian (debug): g_w and the anchored H_w of the weights w_in as dpgo_group_ml_hessian hands out its own.
 * dpgo_debug_ml_gnc_edge_host (no GPU): the kernel's arithmetic per edge in graph order given w (num_edges, each in [0, 1]):
 *   r, wr, chi2, grad, jw as above, near_pi over w > 0 and near_pi_all; any output may be NULL. */
typedef struct dpgo_ml_gnc_result {
  dpgo_gnc_result_t gnc;
  long long near_pi, near_pi_all;
} dpgo_ml_gnc_result_t;
int dpgo_group_ml_gnc(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, const dpgo_gnc_options_t *opt,
                      const int *robust_set, long long max_bytes, double *Xout, int ldout, double *weights, double *log, int log_cap,
                      dpgo_ml_gnc_result_t *result);
int dpgo_group_ml_gnc_eval(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int kind, double mu, double barc2,
                           const int *robust_set, const double *w_in, int full, double *chi2, double *w, double *sums, double *r,
                           double *wr, double *grad, double *jw);
int dpgo_group_debug_ml_gnc_hessian(dpgo_group_t *grp, const dpgo_graph_t *graph, const double *X, int ld, int anchor,
                                    const int *robust_set, const double *w_in, int *ptr, int *col, double *val, long long cap,
                                    long long *nnz, double *grad);
int dpgo_debug_ml_gnc_edge_host(const dpgo_graph_t *graph, const double *X, int ld, const double *w, double *r, double *wr,
                                double *chi2, double *grad, double *jw, long long *near_pi, long long *near_pi_all);

/* ---- the Riemannian staircase: escape a NEGATIVE certificate -------------------------------- */
/* When dpgo_group_verify says NEGATIVE the point is a saddle or a local minimum of the rank-d problem, and the unit vector x it
 * returns is a direction of descent one rank up.  dpgo_group_staircase is the loop of SE-Sync (C++/SESync/src/SESync.cpp:280-440,
 * escape_saddle :575-680, round_solution) on the device.  A point at rank r, d <= r <= 2d, is (d+1)N x r in the reference's row
 * order with Y_p Y_p^T = I_d; F = 1/2 tr(Y^T M Y), grad F = S Y, Hess[V] = Proj_Y(S V), the retraction is the polar factor.
 *     r = d;  Y = X
 *     repeat:  Y = TNT(Y) at rank r     (the reference's truncated-Newton trust-region method; preconditioner Proj o T_p o Proj
 *                                        with the certificate's block-Jacobi T_p)
 *              verdict, theta, x = verify at Lambda(Y)     (Cholesky of S + eta I, then LOBPCG only when it did not succeed)
 *              verdict != NEGATIVE -> SOLVED;   r == r_max -> MAX_RANK
 *              Ydot = x in the zero column r;  alpha = 1; at most 30 times: Z = retract(Y, alpha Ydot), accepted when
 *              F(Z) <= F(Y) + 1/4 alpha^2 theta, else alpha /= 2;   none accepted -> SADDLE;   Y = Z, r += 1
 *     round:   B = the d leading eigenvectors of sum_p Y_p^T Y_p, each signed so that its entry of largest magnitude is positive;
 *              Xhat = Y B with every Y_p B projected onto SO(d), the last column of B negated first where most determinants are
 *              negative (at final rank d the point is taken as it is)
 *     Xhat = polish(Xhat) (opt->polish, anchor 0; left alone where the polish is SKIPPED)
 *     F(Xhat) > F(X) -> Xhat = X, replaced_by_input = 1:  the result is never worse than what was handed in
 * Deviations from the reference: the escape's line search (the reference starts at 10 tol / |theta| and adds a gradient test),
 * r_max <= 2d (the reference: 10), the start at rank d from the caller's point (the reference: r0 = 5 from chordal).
 * The restrictions of the certificate: the TRIVIAL LOSS only, the group must HOST EVERY NODE; -1 otherwise.  The optimiser's
 * state is not touched.
 *   opt     NULL: the defaults.  The optimiser's options are named as in SESyncOpts; r_max 0 means 2d, and must lie in [d, 2d]
 *   Xhat    (d+1) N x d column-major, ldx >= (d+1) N (not written for SKIPPED)
 *   Y       optional, (d+1) N x 2d, ldy >= (d+1) N: the final lifted point, zero columns >= final_rank
 *   log     optional, log_cap rows of 10 doubles, one per level: rank, F in, F out, |grad|, TNT iterations, Hessian products,
 *           certificate status, theta, accepted alpha (0: no escape from this level), halvings
 *   result  outcome; cert_status, theta, stationarity (|grad F| at the final Y) of the last verify; final_rank, levels; the
 *           TNT iterations and Hessian products of all levels; F_initial (at X), F_sdp (at the final Y), F_rounded (before
 *           the polish), F_final (at Xhat); gap = F_final - F_sdp; sigma: the 2d singular values of the rotation rows of the
 *           final Y, descending (more than d of them away from zero: the relaxation is not tight); replaced_by_input;
 *           polish_outcome; device_bytes (filled for SKIPPED too); optimise_ms, verify_ms, round_ms (with the polish), total_ms
 * gap is the reference's suboptimality_bound: F_sdp bounds F of EVERY feasible point from below -- so gap bounds how far Xhat
 * is from the global minimum -- only where cert_status is PROVEN and stationarity is small.  Otherwise it is the difference
 * of two numbers.
 * SKIPPED when the record arrays this allocates (device_bytes) are more than max_bytes (> 0) or more than half of the free
 * device memory: nothing is allocated then. */
#define DPGO_STAIR_SOLVED 0
#define DPGO_STAIR_MAX_RANK 1
#define DPGO_STAIR_SADDLE 2
#define DPGO_STAIR_SKIPPED 3
typedef struct dpgo_staircase_options {
  double grad_norm_tol, preconditioned_grad_norm_tol, rel_func_decrease_tol, stepsize_tol;   /* 1e-2, 1e-4, 1e-6, 1e-3 */
  int max_iterations, max_tCG_iterations;   /* 1000, 10000 */
  double STPCG_kappa, STPCG_theta;          /* 0.1, 0.5 */
  int r_max, precondition;                  /* 0 (2d), 1 */
  int polish, reserved;                     /* 1 */
  double min_eig_num_tol;                   /* 1e-3: eta of the certificate */
  long long max_factor_bytes;               /* 0: of verify's factorisation */
} dpgo_staircase_options_t;
typedef struct dpgo_staircase_result {
  int outcome, cert_status, final_rank, levels;
  int tnt_iterations, hess_products, replaced_by_input, polish_outcome;
  double theta, stationarity, F_initial, F_sdp, F_rounded, F_final, gap;
  double sigma[6];
  long long device_bytes;
  double optimise_ms, verify_ms, round_ms, total_ms;
} dpgo_staircase_result_t;
void dpgo_staircase_options_default(dpgo_staircase_options_t *opt);
int dpgo_group_staircase(dpgo_group_t *grp, const double *X, int ld, const dpgo_staircase_options_t *opt, long long max_bytes,
                         double *Xhat, int ldx, double *Y, int ldy, double *log, int log_cap, dpgo_staircase_result_t *result);
/* Operator hooks on a lifted point Y handed in as (d+1) N x 2d with zero columns >= r (tests/test_gpu_stair_ops.py):
 *   eval     F, |grad F|, Lambda (optional: N blocks d x d row-major by global pose), grad = S Y (optional, (d+1) N x 2d)
 *   hess     out = Hess[V] = Proj_Y(S V)
 *   retract  Z = the polar retraction of Y + V
 *   round    B (2d x d row-major), sigma (2d), Xhat ((d+1) N x d) before any polish */
int dpgo_group_stair_eval(dpgo_group_t *grp, const double *Y, int ldy, double *F, double *grad_norm, double *Lambda, double *grad,
                          int ldg);
int dpgo_group_stair_hess(dpgo_group_t *grp, const double *Y, int ldy, const double *V, int ldv, double *out, int ldo);
int dpgo_group_stair_retract(dpgo_group_t *grp, const double *Y, int ldy, const double *V, int ldv, double *Z, int ldz);
int dpgo_group_stair_round(dpgo_group_t *grp, const double *Y, int ldy, double *B, double *sigma, double *Xhat, int ldx);

/* Host only: the Rayleigh-Ritz step of the search (LOBPCG.h:236-262).  A, B: n x n row-major symmetric, n = ns nblk.
 * Both are scaled by diag(B)^-1/2, B is Cholesky-factored -- a pivot below 1e-12 drops the last block and the step is
 * redone on the others -- and the reduced problem is solved by cyclic Jacobi.  theta: the ns smallest Ritz values; C:
 * n x ns row-major with C^T B C = I, C^T A C = diag(theta), rows of dropped blocks zero; *used: blocks used. */
int dpgo_debug_rayleigh_ritz(int ns, int nblk, const double *A, const double *B, double *theta, double *C, int *used);

/* ---- test hooks ------------------------------------------------------------------------- */
/* Host: the assembled operator `name` in {"G","S","P","P0","Q","D"} of a node as COO triplets in
 * the REFERENCE row/column order.  Call with rows == NULL to get the count. */
int dpgo_debug_node_matrix(const dpgo_graph_t *g, int node, const dpgo_options_t *opt, const char *name,
                           int *rows, int *cols, double *vals);
/* Host: the proximal coefficients T (n0), N (n0 x d), V (n0 x d x d). */
int dpgo_debug_node_proximal(const dpgo_graph_t *g, int node, const dpgo_options_t *opt, double *T, double *N,
                             double *V);
/* Host: multifrontal factor + solve of a CSR SPD matrix, X (n x ncols row-major) <- A^-1 X. */
int dpgo_debug_spd_solve(int n, const int *ptr, const int *col, const double *val, double *X, int ncols,
                         int leaf);
/* Host: size of the multifrontal factor of a CSR SPD matrix for a given nested-dissection leaf size. */
int dpgo_debug_spd_stats(int n, const int *ptr, const int *col, const double *val, int leaf, long *nnz, int *levels,
                         int *max_front);
/* The factor itself, front by front (tests/test_factor_fronts_host.py, tests/test_gpu_factor_fronts.py).  Bypasses nothing:
 * spd_factor(A, F, leaf, collapse, block) as a group calls it (quiet: a non-positive pivot is an answer, nothing is
 * printed), the numeric phase on the device where there is one (DPGO_SPD_HOST_FACTOR=1 or no device: the host loop).
 * refactor_val (optional): a second value array of the same pattern, factored after the first through the KEPT context
 *   (keep_device + keep_numeric, the values copied into spd_numeric_values, spd_refactor_device: the path of a Dynamic
 *   rescale and of the certificate); without a device spd_refactor's host path.
 * factor_only: the certificate's route (spd_symbolic, spd_prepare_device, spd_refactor_device; collapse < 1 counts as 1):
 *   the verdicts and the pivot ranges only, W / WT are never allocated.  Without a device: spd_factor, W / WT dropped.
 * Returns 0 and a handle when every factorisation ended with a verdict, -1 on an error.
 * dpgo_debug_spd_factor_get copies out what the handle holds; every pointer may be NULL:
 *   sizes[8]    nfronts, |upd_idx|, |W|, |WT| (doubles, padding included), doubles held of the first factor's W (0: failed
 *               or factor_only), of the second, whether a second factorisation ran, whether the device numeric phase ran
 *   status[4]   first verdict (0 factored, 1 not positive definite), the front the numeric phase named (-1: none); the same
 *               for the second factorisation (-1, -1 when none ran)
 *   pivots[4]   pivot_min, pivot_max of the first and of the second factorisation
 *   fronts      6 ints per front: w, u, parent, height, ldw, ldm;  offsets: 2 per front: w_off, wt_off
 *   piv_idx     n matrix indices, the fronts' pivots one after the other (the elimination order: fronts are in post-order)
 *   upd_idx     the fronts' update rows one after the other (u each)
 *   W, WT       SpdFactor::W / WT as the first numeric phase left them; W2, WT2: the second's */
typedef struct dpgo_spd_debug dpgo_spd_debug_t;
int dpgo_debug_spd_factor(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int factor_only, dpgo_spd_debug_t **out);
int dpgo_debug_spd_factor_get(const dpgo_spd_debug_t *h, long long *sizes, int *status, double *pivots, int *fronts,
                              long long *offsets, int *piv_idx, int *upd_idx, double *W, double *WT, double *W2, double *WT2);
void dpgo_debug_spd_factor_free(dpgo_spd_debug_t *h);
/* Selected inversion of a given SPD CSR matrix, front by front (tests/test_covariance_host.py, tests/test_gpu_selinv_fronts.py):
 * the entries of A^-1 inside the factor's pattern from the explicit W_s = [L11^-1 ; -L21 L11^-1] (spd.h: spd_selinv_*).
 * spd_factor(A, F, leaf, collapse, block), quiet, then
 *   on the device (host == 0 and a HIP device): keep_device + keep_numeric, spd_selinv_device twice (the second call's
 *     blocks are kept beside the first's), then spd_refactor_device from the SAME values (W before the inversion and after
 *     this factorisation are both kept) and, with refactor_val, from the second values through the kept context and
 *     spd_selinv_device again;
 *   on the host (host != 0, or no device): spd_selinv_host on the factor's W, and with refactor_val spd_refactor and
 *     spd_selinv_host again.
 * A factorisation that meets a non-positive pivot is not inverted: its verdict is 1 and its blocks are not there.
 * Returns 0 and a handle when every step ended with a verdict, -1 on an error or a bad argument.
 * dpgo_debug_spd_selinv_get copies out what the handle holds; every pointer may be NULL:
 *   sizes[8]    nfronts, |upd_idx|, doubles of all S_front (sum of (w + u)^2), doubles held of the first inversion (0: not
 *               inverted), of its repetition, of the second values' inversion, doubles of W held before / after, whether the
 *               device ran (sizes[7])
 *   status[4]   verdict of the first factorisation (0 factored, 1 not positive definite), of its inversion (0 done, 1 refused
 *               because not positive definite), the same two for the second values (-1, -1 when none were given)
 *   pivots[4]   pivot_min, pivot_max of the first and of the second factorisation
 *   fronts      4 ints per front: w, u, parent, depth;  piv_idx, upd_idx: as dpgo_debug_spd_factor_get gives them
 *   sigma, sigma_again, sigma2   S_front of every front one after the other, (w + u) x (w + u) row-major, pivots first
 *   W_before, W_after            SpdFactor::W (padding included) of the first factorisation and of the one behind the inversion */
typedef struct dpgo_spd_selinv_debug dpgo_spd_selinv_debug_t;
int dpgo_debug_spd_selinv(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, dpgo_spd_selinv_debug_t **out);
int dpgo_debug_spd_selinv_get(const dpgo_spd_selinv_debug_t *h, long long *sizes, int *status, double *pivots, int *fronts,
                              int *piv_idx, int *upd_idx, double *sigma, double *sigma_again, double *sigma2,
                              double *W_before, double *W_after);
void dpgo_debug_spd_selinv_free(dpgo_spd_selinv_debug_t *h);
/* The device solve for ONE plain vector on a given SPD CSR matrix (tests/test_polish_host.py, tests/test_gpu_vsolve_fronts.py):
 * spd_factor(A, F, leaf, collapse, block), quiet, then
 *   on the device (host == 0 and a HIP device): keep_device + keep_numeric, spd_vsolve_device on a copy of rhs, twice;
 *   on the host (host != 0, or no device): spd_solve_host, twice;
 * and with refactor_val the second values through the kept context (spd_refactor_device; on the host spd_refactor) and one
 * more solve.  out holds 3 n doubles: the first solution, its repetition, the second values' solution.  A part whose
 * factorisation met a non-positive pivot is not written.
 *   status[2]   verdict of the first factorisation (0 factored, 1 not positive definite) and of the second (-1: none given)
 *   pivots[4]   pivot_min, pivot_max of the first and of the second factorisation
 * Returns 1 when the device ran, 0 when the host did, -1 on an error or a bad argument. */
int dpgo_debug_spd_vsolve(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, const double *rhs, double *out, int *status, double *pivots);
/* How many entries of a front's input vector spd_vsolve_device stages in LDS at a time: 1 ... 2048, anything else restores the
 * default 2048.  Process-wide; returns the value before.  For the tests: a chunk's edge inside fronts of a few hundred rows. */
int dpgo_debug_spd_vsolve_chunk(int chunk);
/* The device solve for a BLOCK of k plain vectors on a given SPD CSR matrix (tests/test_msolve_host.py,
 * tests/test_gpu_msolve_fronts.py): dpgo_debug_spd_vsolve's sequence with spd_msolve_device(F, X, k, ldx) on the device and
 * spd_solve_host(F, X, k) on the host.  rhs is n x k row-major.  out holds 3 n ldx doubles, three n x ldx row-major arrays:
 * the first solution, its repetition, the second values' solution.  On the device each is uploaded as the caller filled it
 * with rhs written into its first k columns, solved in place and read back whole, so the entries (i, k ... ldx) show what
 * the solve left there; on the host only the first k columns are written.  A part whose factorisation met a non-positive
 * pivot is not written.
 *   chunk       > 0: for the length of the call, how many rows of a front's input block the device stages in LDS at a time
 *               (spd_msolve_chunk: 1 ... 32, anything above restores the default 32); <= 0: as it is
 *   status, pivots, the return value: as dpgo_debug_spd_vsolve; -1 also for k < 1 or ldx < k. */
int dpgo_debug_spd_msolve(int n, const int *ptr, const int *col, const double *val, const double *refactor_val, int leaf,
                          int collapse, int block, int host, int chunk, const double *rhs, int k, int ldx, double *out,
                          int *status, double *pivots);
/* The device solve on a given matrix (tests/test_gpu_solve_tiles.py): an SpdSolverDev built as a group builds its own --
 * spd_factor(A, F, leaf, collapse, block) with the factor left on the device unless DPGO_SPD_DEVICE_PANELS=0, then
 * upload(dof, d, node_of_unknown) -- and spd_run on it.  The hook calls what exists; it adds nothing to spd_run or the kernels.
 * create    d in {2, 3}, dof in {1, d} (1: unknown i is the translation row of record i; d: the rotation row i % d of record
 *           i / d), node_of_unknown[n]: the local node (< 64) of every unknown -- unknowns of different nodes must not be
 *           coupled; keep_numeric: the numeric context stays (a Dynamic rescale's G_tt), which refactor needs.
 *           Returns 0, -1 on a bad argument or a failed factorisation, -2 without a HIP device (nothing is touched).
 * plan      what upload() decided; every pointer may be NULL.  L = sizes[2] + sizes[3] + 3 launches: the forward levels, the
 *           backward levels, then the fused roots, their finer class and the triangle's block rows.
 *   sizes[8]     nfronts, |upd_idx|, forward levels, backward levels, local nodes, n, doubles of a record array, stored entries
 *   flags[8]     fused_root, root_sym, tile height of the roots, root_fine_rows, root_fine_below, stream_once, dof, d
 *   levels       3 ints per launch: rows (height of its wide tiles), nwide, nnarrow
 *   node_counts  per launch and local node 2 ints: wcount, ncount
 *   fronts       4 ints per front: w, u, parent, height;  piv_idx / upd_idx as dpgo_debug_spd_factor_get gives them
 * fine_root 1 / 0: SpdSolverDev::fine_root_for(nodes)
 * run       in, out: host record arrays, (d + 1) x d doubles per record.  out is uploaded first (the solve writes the
 *           unknowns of the live nodes and nothing else) and read back.  mask_word (optional): the value of the device mask
 *           word (NodeMask::p); class_of (optional): the node set the roots' tile class is chosen for; scale: +1 or -1;
 *           in_place: in == out on the device (out receives the array).  Returns 0, -1 on an error, -2 when spd_run itself
 *           refuses (in place with fused roots).
 * refactor  new values (the order of create's val) to the device, spd_refactor_device, repack().  Returns 0, 1 when the new
 *           matrix is not positive definite, -1 on an error (also: created without keep_numeric). */
typedef struct dpgo_spd_solver_debug dpgo_spd_solver_debug_t;
int dpgo_debug_spd_solver_create(int n, const int *ptr, const int *col, const double *val, int leaf, int collapse, int block,
                                 int d, int dof, const int *node_of_unknown, int keep_numeric, dpgo_spd_solver_debug_t **out);
int dpgo_debug_spd_solver_plan(const dpgo_spd_solver_debug_t *h, long long *sizes, int *flags, int *levels, int *node_counts,
                               int *fronts, int *piv_idx, int *upd_idx);
int dpgo_debug_spd_solver_fine_root(const dpgo_spd_solver_debug_t *h, unsigned long long nodes);
int dpgo_debug_spd_solver_run(dpgo_spd_solver_debug_t *h, unsigned long long mask_v, const unsigned long long *mask_word,
                              const unsigned long long *class_of, double scale, int in_place, const double *in, double *out);
int dpgo_debug_spd_solver_refactor(dpgo_spd_solver_debug_t *h, const double *val);
void dpgo_debug_spd_solver_free(dpgo_spd_solver_debug_t *h);
/* Host: one solve tile's panel as SpdSolverDev::upload's host packer lays it out.  The tile has `count` rows in the class of
 * `rows`-high tiles (64, 16 or 8: 1, 4 or 8 lanes per row) and `len` entries per row; entry (k, r) is src[k * src_ld + r];
 * pairs: what DPGO_SPD_PANEL_PAIRS would be.  info[4] = the descriptor's ld, its pair_kq (0: plain layout, else lanes per
 * row of the paired one), its mat_off (the one given), doubles of the panel.  panel (may be NULL to query info): at least
 * mat_off + info[3] doubles; the packer writes the entries and nothing else.  Returns 0, -1 on a bad argument. */
int dpgo_debug_spd_panel_pack(int rows, int count, int len, int pairs, long long mat_off, const double *src, int src_ld,
                              double *panel, long long cap, long long *info);
/* Host: the neighbour-to-neighbour exchange plan of `rank` (what dpgo_comm_exchange uses with more than one rank) from
 * every rank's exported and needed (node, pose) keys (dpgo_graph_exchange_plan of its nodes): per peer 5 ints (rank,
 * send_off, send_cnt, recv_off, recv_cnt), the send and receive keys (node, pose interleaved, concatenated over the peers
 * in the order both ends agree on: ascending (node, pose)); sizes[0..2] = peers, send keys, receive keys.  Output
 * pointers may be NULL to query the sizes. */
int dpgo_debug_p2p_plan(int rank, int nranks, const int *exp_counts, const int *exp_nodes, const int *exp_poses,
                        const int *need_counts, const int *need_nodes, const int *need_poses, int *peers, int *send_keys,
                        int *recv_keys, int *sizes);
/* Device: single operators of one node on reference-layout inputs:
 *  "project" (d n0 x d -> nearest rotations), "solve_tt" ((d+1) n0 x d, translation rows),
 *  "solve_rr" (rotation rows), "G" ((d+1) n0 x d -> G X), "proximal" (in = [Z ; Df] stacked),
 *  "hess" (in = [Y ; nabla ; Ydot ; r] -> Hessian-vector product and 4 CG sums), "rgrad" (in = [Y ; g] -> both gradient
 *  paths), "precon" (in = [Y ; v]), "retract" (in = [Y ; Ydot ; g]), "lambda_max" (out[0]); Group::debug_apply lists the
 *  layouts.  A suffix ":all" runs the operator under the whole group's launch mask. */
int dpgo_group_debug_apply(dpgo_group_t *grp, int local, const char *op, const double *in, int ld_in,
                           double *out, int ld_out);
/* Device: the scalar kernels of the truncated CG (the step length, the boundary / negative-curvature / kernel exits, the
 * stopping tests, the three device masks) on GIVEN partial sums.  A script of n launches, each made by its production
 * launcher on the group's own records, masks, pinned summaries and read-back flag:
 *   kind 0 begin_host  (bits, rv, Delta, target, max_it)           the start values of a later round
 *        1 begin_device (bits, Delta, use_precon, max_it, the tolerances; sums in slots 0..3 and 6, 7)
 *        2 scal0 / 3 scal1   phase 0 (slots 0..3) / phase 1 (slot 0) of a CG step
 *        4 scal_begin   begin_device and phase 0 in one launch (the step's four sums from slot 16 on)
 * partials: slots x nseg_all doubles (slot-major), copied over the partial sums before the launch (slots = 0: left alone);
 * dpgo_group_debug_seg_layout gives nseg_all and, per local node a, its own segments [own_ptr[a], own_ptr[a+1]) and
 * neighbour segments [nbr_ptr[a], nbr_ptr[a+1]).  rv, Delta, target: one double per local node.
 * Read back after every launch i (L = the group's nodes): records[i][a][17] -- sk_M_pk, sk_M_2, pk_M_2, rv, Delta, Delta_2,
 * target, h_M_norm, c1, cr, al, kap, be, cg_it, max_it, live, stop_ord --, masks[i][3], cg_summary[i][a][4] (stop ordinal or
 * 1e18 while live, h_M_norm, cg_it, unused), tnt_summary[i][a][8] and dev_tnt[i][a][8] (the six start sums, active, unused:
 * pinned and device copies), seq[i][2] (the flag's value, the last sequence number given out), arrived[i] (the flag's
 * arrival counter: 0 between launches).
 *   kind 5 reduce_gate  the trial point's reduction with the gate of a speculative update behind it, as the iteration launches
 *                       it: gate->nslots sums per node over own rows to the pinned scalars and to their device copy, then the
 *                       gate's verdict from those sums, the refinement's start (what an earlier scal_begin of the script left
 *                       in device memory) and the CG records, against the per-node scalars (f, Fk0, Fk1, fobj, hits0, hits1:
 *                       one per local node) and the options in *gate
 *        6 reduce       the plain reduction over own rows of gate->nslots sums per node (the rest of *gate is not read)
 * After a launch of kind 5 or 6: gate_sums[i][2][a][32] (the pinned scalars, the device copy) and gate_words[i][2] (the gate's
 * device word -- all ones or 0 --, the bits of its pinned verdict, 1.0 or 0.0); both may be NULL in a script without such a launch. */
typedef struct dpgo_gate_debug {
  int nslots, max_it, max_acc, max_hits0, max_hits1;
  double rel_tol, step_tol, psi, phi;
  const double *f, *Fk0, *Fk1, *fobj;
  const int *hits0, *hits1;
} dpgo_gate_debug_t;
typedef struct dpgo_cg_debug_launch {
  int kind, use_precon, max_it, slots;
  unsigned long long bits;
  double grad_tol, pgrad_tol, kappa, theta;
  const double *rv, *Delta, *target, *partials;
  const dpgo_gate_debug_t *gate;   /* kinds 5 and 6 */
} dpgo_cg_debug_launch_t;
int dpgo_group_debug_seg_layout(dpgo_group_t *grp, int *nseg_all, int *own_ptr, int *nbr_ptr);
int dpgo_group_debug_cg_scalars(dpgo_group_t *grp, const dpgo_cg_debug_launch_t *script, int n, double *records,
                                unsigned long long *masks, double *cg_summary, double *tnt_summary, double *dev_tnt,
                                unsigned long long *seq, unsigned *arrived, double *gate_sums, unsigned long long *gate_words);
/* Device: AMM-PGO*'s master sums (k_star_sums, k_publish) on GIVEN partial sums, through the two launches the master's read-back
 * ends with.  partials: 32 x nseg_all doubles (slot-major), copied over the partial sums; valid: bit q (q < 6) = sum q was
 * produced, the six sums being in slots 0, 1, 30, 31, 4, 5.  out[0..3]: F1, F2, d1, d2 as they are in device memory, out[4..7]:
 * as published to the host; seq[2]: the flag's value, the last sequence number given out.  -1: a null pointer, bits of `valid`
 * above 5. */
int dpgo_group_debug_star_sums(dpgo_group_t *grp, const double *partials, unsigned valid, double *out, unsigned long long *seq);
/* Device: the launches an update enqueued ahead of the host's decision consists of -- the local halo copy, the product with G,
 * the inter-edge pass -- under a GIVEN gate word (0: they must fall through; all ones: they run), with the group's buffers in
 * the roles of the accepted step when called between dpgo_group_iterate and dpgo_group_update (as the iteration enqueues
 * them), in their present roles behind an update (the launches then repeat it).  For a group with a robust loss and Static
 * rescale whose every node is past its first iteration; every buffer the launches may write is saved before and put back
 * afterwards, so the group can go on.  report: 3 ints for each of 12 buffers (Xk, X[iter], X[iter-1], g, g[iter-1], Dfobj,
 * Dfobj[iter-1], G X, G X[iter-1], the partial sums, DfobjE, the edge weights): the buffer exists; it is bit-identical to the
 * saved copy after the gated launches; the gated launches' result is bit-identical to that of the same launches without a
 * gate from the same state (all ones only, else -1).  -1: a null pointer, a word other than 0 / all ones, a group in another
 * state. */
int dpgo_group_debug_gated_update(dpgo_group_t *grp, unsigned long long go_word, int *report);
/* Device: ONE truncated CG of a refinement round, and nothing after it, on given points: the model gradient and the norms,
 * the start on the host (device_start = 0: a later round's) or on the device (1: the first round's), the CG steps -- the pieces
 * dpgo_group_iterate's refinement is made of, in its order, with the group's options (max_tCG_iterations, STPCG_kappa,
 * STPCG_theta, the gradient tolerances, the preconditioner).  locals: the n nodes that take part.  in: for EVERY node of the
 * group, in order, [Y ; g] stacked ((d+1) n0 rows each: translations, then rotation rows); Delta: one radius per node of the
 * group.  out: for every node [s ; H s ; grad] (3 (d+1) n0 rows); the work vectors' rows of the nodes outside `locals` are
 * set to `fill` before the run and come back in `out`.  scalars: 12 per node -- |grad|^2, <Y, nabla>, <Y, g>, <Y, g>,
 * |P grad|^2, <grad, P grad> (the last two 0 without a preconditioner), h_M_norm, cg_it, stop_ord, active, live, Delta
 * (zeros for a node outside `locals`; h_M_norm .. Delta zero for a node that failed a gradient test). */
int dpgo_group_debug_stpcg(dpgo_group_t *grp, const int *locals, int n, const double *in, int ld_in, const double *Delta,
                           int device_start, double fill, double *out, int ld_out, double *scalars);
/* Device: the robust inter-edge pass (k_inter), the objective (k_cost) and the Dynamic rescale on GIVEN inputs, each through
 * the launch the iteration makes (tests/test_gpu_inter.py, tests/test_gpu_rescale_ops.py).  Matrices are reference layout,
 * column-major and contiguous: "all" = (d+1)(n0+n1) x d -- own and neighbour rows of node `local`, [t_own ; R_own ; t_nbr ;
 * R_nbr] --, "own" = (d+1) n0 x d.  whole = 1: under the whole group's launch mask, the other nodes' rows zero.  Robust losses
 * only.  The entries overwrite the group's iterates; use them on a group that does not iterate afterwards.
 * inter_update: update()'s pass at Z.  quad: the majorisation gap against Zprev and the previous DfE (DfE_old); with_Df: Dfobj =
 *   GX + g, its tangent projection at X and |grad F|^2 (sums[4]) -- 1: inside the pass, 2: by k_tangent_full behind it; Znbr (optional, all): the neighbour rows are read from it
 *   and copied into Z on the way (the halo copy); recv / nrecv / nsrc (optional, with Znbr): a lazy unpack -- recv holds nrecv
 *   poses ((d+1) nrecv x d: translations, then rotation blocks), nsrc[r] the slot of neighbour row r or -1.  Out: DfE (all),
 *   g (own), w (one weight per inter-node edge of the node, in the order of its measurements), sums[5] (slots 0..4: sum rho,
 *   the quad term, <z, g>, unused, |grad F|^2), Df (own, with_Df), Z_after / Znbr_after (all, optional): what the pass left.
 * inter_iterate: iterate()'s pass at Y = Zc + gamma[node] (Zc - Zp), as prepare_extrapolated enqueues it.  fused = 1: the
 *   extrapolation inside the pass (and, with the kept products GXc / GXp of a statically scaled group, Df; with prox the
 *   proximal half step on it); fused = 0: the extrapolation, the pass and the proximal step as launches of their own.
 *   gamma_dev = 1: the gammas are read from device memory.  Out: Y (all; a fused pass stores its own rows only), g, Df (own),
 *   Xout and Xref_after (own, with prox: proximal(Y, Df), and Xref with Xout's rotations), sums[2] = <Y, g>, |Xout - Xref|^2.
 * cost: k_cost at Z (all): sums[2] = the intra-node edges' costs, the inter-node edges' rho; eform 1: the data-matrix form.
 * rescale (Rescale::Dynamic groups): w, scale: one per inter-node edge of the GROUP (node a's start at edge_offsets[a]); count:
 *   one per node; nodes: the set that is tested.  Runs the test, then the rescale of the flagged nodes (the block-diagonal
 *   terms, the factorisation of G_tt, the solve's panels).  Returns the number of rescaled nodes, -1 on an error. */
typedef struct dpgo_inter_update_debug {
  int local, whole, quad, with_Df, nrecv;
  const double *Z, *Zprev, *DfE_old, *GX, *X, *Znbr, *recv;
  const int *nsrc;
  double *DfE, *g, *w, *sums, *Df, *Z_after, *Znbr_after;
} dpgo_inter_update_debug_t;
typedef struct dpgo_inter_iterate_debug {
  int local, whole, fused, prox, gamma_dev;
  const double *Zc, *Zp, *GXc, *GXp, *Xref, *gamma;
  double *Y, *g, *Df, *Xout, *Xref_after, *sums;
} dpgo_inter_iterate_debug_t;
int dpgo_group_debug_inter_update(dpgo_group_t *grp, const dpgo_inter_update_debug_t *q);
int dpgo_group_debug_inter_iterate(dpgo_group_t *grp, const dpgo_inter_iterate_debug_t *q);
int dpgo_group_debug_cost(dpgo_group_t *grp, int local, int whole, int eform, const double *Z, double *sums);
int dpgo_group_debug_edge_offsets(const dpgo_group_t *grp, int *edge_offsets);   /* num_local + 1 ints */
int dpgo_group_debug_rescale(dpgo_group_t *grp, const double *w, const double *scale, const int *count, int max_rescale_count,
                             const int *nodes, int n, int *flags, double *host_flags, double *scale_out, int *count_out);
/* Device: the kernels of the certificate's LOBPCG search (k_cert_gram, k_cert_update, k_cert_reduce) and the host's block-Jacobi
 * preconditioner on GIVEN inputs, each through the launch dpgo_group_certify's loop makes (tests/test_gpu_cert_search.py).
 * Matrices are (d+1)N x d in the layout of X, column-major with leading dimension ld.  Same restrictions as dpgo_group_certify.
 * cert_gram: Lambda from X; the buffer of S W takes MW (= M W), or, MW null, the product M W the loop forms.  One gram launch,
 *   one reduction.  sums: 2 ntri + 2 d doubles, ntri = 3d (3d + 1) / 2 -- the row-major upper triangles of B^T B, then of
 *   B^T (S B) (entry (a, c), a <= c: B_a^T (S B)_c; B = [V W P], S B = [SV SW SP]), then 2 d the launch does not write; SW:
 *   the finished S W = M W - [0 ; Lambda W_Y].
 * cert_update: C (3d x d row-major: the rows of V, W, P) and theta[d]; precondition 1: W' = T_p R', 0: W' = R'.  One update
 *   launch, one reduction.  The outputs are the six buffers afterwards (SW is read only); sums as above, the last 2 d are
 *   |R'_j|^2 and |V'_j|^2; the neighbour records of V, W, P (dpgo_group_debug_cert_nbr_rows() of (d+1) d doubles each, which
 *   the launch must leave alone) are set to nbr_fill before it and come back raw in nbr (three runs: V's, W's, P's).
 * cert_precon: the blocks T_p the search applies, N x (d+1) x (d+1) by global pose (slot 0 the translation).
 * cert_trace: with on = 1 every later search of the group (certify, verify, the staircase's) records one entry per pass of
 *   its loop that reached the update -- the sums it read, nblk, used, theta[d], the C it passed on (3d x d), and 1.0 where a
 *   refresh of S V, S P followed: record_len = 2 ntri + 2 d + 2 + d + 3 d d + 1 doubles --; cert_trace_get hands out the
 *   records of the last search (records null: the sizes alone).  Off (the default) the search does nothing for it. */
typedef struct dpgo_cert_update_debug {
  const double *C, *theta, *V, *W, *P, *SV, *SW, *SP;
  int ld, precondition;
  double nbr_fill;
  double *V_out, *W_out, *P_out, *SV_out, *SW_out, *SP_out, *sums, *nbr;
} dpgo_cert_update_debug_t;
int dpgo_group_debug_cert_gram(dpgo_group_t *grp, const double *X, const double *V, const double *W, const double *P,
                               const double *SV, const double *SP, const double *MW, int ld, double *sums, double *SW);
int dpgo_group_debug_cert_update(dpgo_group_t *grp, const dpgo_cert_update_debug_t *q);
int dpgo_group_debug_cert_nbr_rows(const dpgo_group_t *grp);
int dpgo_group_debug_cert_precon(dpgo_group_t *grp, double *T);
int dpgo_group_debug_cert_trace(dpgo_group_t *grp, int on);
int dpgo_group_debug_cert_trace_get(const dpgo_group_t *grp, double *records, long long cap, int *record_len, long long *count);

#ifdef __cplusplus
}
#endif
#endif /* DPGO_AMD_H */
