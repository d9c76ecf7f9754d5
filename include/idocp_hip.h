/*
 * idocp_hip.h -- C ABI of the MI355X-native KKT-condensation + Riccati hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI:
 * its boundary is the C++ classes idocp::Robot (include/idocp/robot/robot.hpp:26),
 * idocp::UnOCPSolver (include/idocp/unocp/unocp_solver.hpp:25-188) and
 * idocp::OCPSolver (include/idocp/ocp/ocp_solver.hpp).  The C++ facade in
 * include/idocp/ *.hpp keeps those class names / method names and forwards every
 * call to the functions declared here; each entry point cites the reference
 * method it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types
 *   - every function returns an int status: 0 ok, <0 bad argument / runtime
 *     failure (IDOCP_E_*), >0 numerical failure (1 + index of the failing stage)
 *   - caller-owned host buffers, library-owned device buffers; one HIP stream
 *     per handle; a handle is thread-compatible (one caller at a time)
 *   - all arithmetic is IEEE FP64; matrices crossing the ABI are column-major
 *     (the reference's Eigen default)
 *   - "batch" = number of independent OCP instances solved side by side by one
 *     handle (the data-parallel axis of the throughput metric).  batch == 1
 *     reproduces one reference solver object.
 */
#ifndef IDOCP_HIP_H_
#define IDOCP_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define IDOCP_MAX_JOINTS 16
#define IDOCP_MAX_NV 24
#define IDOCP_MAX_NQ 25
#define IDOCP_MAX_CONTACTS 4

#define IDOCP_OK 0
#define IDOCP_E_ARG (-1)      /* invalid argument (reference: throw + std::exit) */
#define IDOCP_E_IO (-2)       /* URDF could not be read / parsed                   */
#define IDOCP_E_DEVICE (-3)   /* HIP runtime error, no GPU, or extension missing   */
#define IDOCP_E_UNSUPPORTED (-4)

#define IDOCP_JOINT_REVOLUTE 0
#define IDOCP_JOINT_FREEFLYER 1

/*
 * Flat rigid-body model: what pinocchio::Model holds for the reference
 * (src/robot/robot.cpp:8-85).  Joint i (0-based) is pinocchio joint i+1; the
 * universe is parent -1.  Spatial vectors are (linear, angular) like
 * pinocchio::Motion / Force.  Rotations are row-major 3x3.
 */
typedef struct idocp_model {
  int njoints;
  int nq, nv, nu;              /* nu = nv - dim_passive                           */
  int has_floating_base;       /* joint 0 is a free-flyer (q: xyz + quat xyzw)    */
  int parent[IDOCP_MAX_JOINTS];
  int jtype[IDOCP_MAX_JOINTS];
  int idx_q[IDOCP_MAX_JOINTS];
  int idx_v[IDOCP_MAX_JOINTS];
  double axis[IDOCP_MAX_JOINTS][3];   /* revolute axis in the joint frame          */
  double plc_R[IDOCP_MAX_JOINTS][9];  /* joint placement in the parent joint frame */
  double plc_p[IDOCP_MAX_JOINTS][3];  /*   x_parent = R x_joint + p                */
  double mass[IDOCP_MAX_JOINTS];      /* body inertia (fixed children merged):     */
  double com[IDOCP_MAX_JOINTS][3];    /*   centre of mass in the joint frame       */
  double inertia[IDOCP_MAX_JOINTS][9];/*   rotational inertia about the com        */
  double gravity[3];                  /* (0, 0, -9.81)                             */
  double q_min[IDOCP_MAX_NV];         /* limits of the nu actuated joints          */
  double q_max[IDOCP_MAX_NV];         /* (reference: Robot::initializeJointLimits, */
  double v_max[IDOCP_MAX_NV];         /*  include/idocp/robot/robot.hxx:699-709)   */
  double u_max[IDOCP_MAX_NV];
  int ncontacts;                      /* point contacts (robot.cpp:66-70)          */
  int contact_frame_id[IDOCP_MAX_CONTACTS]; /* pinocchio frame index               */
  int contact_joint[IDOCP_MAX_CONTACTS];    /* parent joint of the contact frame   */
  double contact_R[IDOCP_MAX_CONTACTS][9];  /* frame placement in that joint frame */
  double contact_p[IDOCP_MAX_CONTACTS][3];
  double total_mass;
} idocp_model_t;

/*
 * ConfigurationSpaceCost (src/cost/configuration_space_cost.cpp:241-397), the
 * cost of configs C1/C2.  Unset weights are zero like the reference's ctor.
 */
/* One more task-space cost component of idocp_cost_t (task_extra): the fields of the task_* block of the cost, per component. */
#define IDOCP_MAX_EXTRA_TASKS 3
typedef struct idocp_task_component {
  int dim;                     /* 3 or 6 */
  int joint;                   /* parent joint of the frame */
  double frame_R[9];           /* placement of the frame in the joint frame, row-major */
  double frame_p[3];
  double weight[6], weightf[6], weighti[6];      /* stage, terminal, impulse-stage weights (layout of task_weight) */
  double ref[12];              /* constant reference: rotation (row-major, 9) then position (3) */
} idocp_task_component_t;

typedef struct idocp_cost {
  double q_ref[IDOCP_MAX_NQ];
  double v_ref[IDOCP_MAX_NV];
  double u_ref[IDOCP_MAX_NV];
  double q_weight[IDOCP_MAX_NV];
  double v_weight[IDOCP_MAX_NV];
  double a_weight[IDOCP_MAX_NV];
  double u_weight[IDOCP_MAX_NV];
  double qf_weight[IDOCP_MAX_NV];
  double vf_weight[IDOCP_MAX_NV];
  /* ContactForceCost (src/cost/contact_force_cost.cpp:153-194): per contact */
  double f_weight[IDOCP_MAX_CONTACTS][3];
  double f_ref[IDOCP_MAX_CONTACTS][3];
  /* TrottingConfigurationSpaceCost (include/idocp/cost/trotting_configuration_space_cost.hpp:
   * 126-164): when use_trotting_ref != 0, q_ref holds q_standing and the reference
   * of stage time t is generated on the host; v_ref[0] = step_length / t_period. */
  int use_trotting_ref;
  double t_start, t_period, step_length;
  double front_swing_knee, hip_swing_knee, front_stance_knee, hip_stance_knee;
  /* Impulse-stage terms (computeImpulseCostDerivatives / Hessian of the same components,
   * src/cost/trotting_configuration_space_cost.cpp:308-376, contact_force_cost.cpp:167-211):
   * weights on q, v, dv and on the impulse forces.  Only used by horizons with impulse events. */
  double qi_weight[IDOCP_MAX_NV];
  double vi_weight[IDOCP_MAX_NV];
  double dvi_weight[IDOCP_MAX_NV];
  double fi_weight[IDOCP_MAX_CONTACTS][3];
  double fi_ref[IDOCP_MAX_CONTACTS][3];
  /* TimeVaryingConfigurationSpaceCost (include/idocp/cost/time_varying_configuration_space_cost.hpp:98-118,
   * src/cost/time_varying_configuration_space_cost.cpp:58-85): when use_time_varying_ref != 0, q_ref holds q_begin,
   * v_ref the constant reference velocity; the reference of stage time t is q_begin for t <= tv_t_begin,
   * q_begin (+) (t - tv_t_begin) v_ref inside (tv_t_begin, tv_t_end) and q_begin (+) (tv_t_end - tv_t_begin) v_ref after;
   * the velocity reference is v_ref inside the window and zero outside. */
  int use_time_varying_ref;
  double tv_t_begin, tv_t_end;
  /* TaskSpace3DCost / TaskSpace6DCost and their TimeVarying variants (src/cost/task_space_{3d,6d}_cost.cpp,
   * time_varying_task_space_{3d,6d}_cost.cpp) on one frame: of a fixed-base robot (UnOCPSolver, also the TimeVarying variants) or of a
   * floating-base one (OCPSolver and ParNMPCSolver on any chain, horizons with discrete events included; constant reference here, the
   * TimeVarying variants through idocp_ocp_set_task_refs; the frame sits on the base or on a link of a leg).  SURVEY 8f row 3.
   * task_dim 0: none; 3: l = 1/2 dt |p_frame(q) - p_ref|^2_W; 6: l = 1/2 dt |log6(M_ref^-1 M_frame(q))|^2_W with the
   * Gauss-Newton Hessian of the reference.  The frame is given by its parent joint and its placement in that joint's
   * frame (idocp_model_frame_placement). */
  int task_dim;
  int task_joint;
  double task_frame_R[9];        /* row-major */
  double task_frame_p[3];
  double task_weight[6];         /* 3D: q_3d_weight; 6D: the vector the reference stores, [rotation_weight; position_weight], which
                                  * multiplies log6 = [linear; angular] entry by entry (time_varying_task_space_6d_cost.cpp:33-38, 60-62) */
  double task_weightf[6];        /* terminal weights (qf_3d_weight / qf_6d_weight), same layout */
  double task_ref[12];           /* constant reference: rotation (row-major, 9) then position (3); 3D uses the position only */
  int task_time_varying;         /* != 0: the references of the N + 1 stages come from idocp_unocp_set_task_refs */
  double task_weighti[6];        /* impulse-stage weights (qi_3d_weight / qi_6d_weight), same layout: OCPSolver on chains with impulse stages */
  /* Further task-space components (CostFunction::push_back takes any number of components, include/idocp/cost/cost_function.hpp:67;
   * round 6): up to IDOCP_MAX_EXTRA_TASKS more TaskSpace3DCost / TaskSpace6DCost terms, each on a frame of its own, summed with the one
   * above.  Constant references (the TimeVarying variants: the first component only).  task_extra_count > 0 needs task_dim != 0. */
  int task_extra_count;
  idocp_task_component_t task_extra[IDOCP_MAX_EXTRA_TASKS];
} idocp_cost_t;

/*
 * Inequality constraints handled by the primal-dual interior point method
 * (include/idocp/constraints/pdipm.hxx:13-87).  The six joint-limit components
 * are what JointConstraintsFactory::create() pushes
 * (src/utils/joint_constraints_factory.cpp:21-38), in the reference's order:
 * position lower/upper, velocity lower/upper, torque lower/upper.
 */
typedef struct idocp_constraints {
  int joint_position_limits;   /* 0/1 */
  int joint_velocity_limits;   /* 0/1 */
  int joint_torque_limits;     /* 0/1 */
  int linearized_friction_cone;/* 0/1: LinearizedFrictionCone (src/constraints/linearized_friction_cone.cpp) */
  double mu;                          /* friction coefficient                     */
  double barrier;                     /* default 1.0e-04 */
  double fraction_to_boundary_rate;   /* default 0.995   */
  int linearized_impulse_friction_cone; /* 0/1: LinearizedImpulseFrictionCone on impulse stages
                                         * (src/constraints/linearized_impulse_friction_cone.cpp), same mu */
  int friction_cone;                    /* 0/1: FrictionCone, two rows per contact: -fz <= 0, fx^2 + fy^2 - mu^2 fz^2 <= 0
                                         * (src/constraints/friction_cone.cpp; the cone of examples/anymal/ocp_benchmark.cpp:76).
                                         * Exclusive with linearized_friction_cone */
  int impulse_friction_cone;            /* 0/1: ImpulseFrictionCone on impulse stages (src/constraints/impulse_friction_cone.cpp).
                                         * Exclusive with linearized_impulse_friction_cone */
  int joint_acceleration_lower_limit;   /* 0/1: JointAccelerationLowerLimit, a.tail(dimu) >= a_min (src/constraints/joint_acceleration_lower_limit.cpp) */
  int joint_acceleration_upper_limit;   /* 0/1: JointAccelerationUpperLimit, a.tail(dimu) <= a_max (src/constraints/joint_acceleration_upper_limit.cpp) */
  double a_min[IDOCP_MAX_NV];           /* the components carry their own bounds (constructor argument amin / amax), one per actuated joint */
  double a_max[IDOCP_MAX_NV];
  int contact_distance;                 /* 0/1: ContactDistance, the frames of the contacts that are NOT active stay above z = 0
                                         * (src/constraints/contact_distance.cpp); floating-base solvers */
} idocp_constraints_t;

/* ---- Robot ------------------------------------------------------------ */

/* Replaces Robot::Robot(path_to_urdf[, contact_frames]) (src/robot/robot.cpp:8-85):
 * reads the URDF and fills *out.  contact_frames are pinocchio frame indices
 * (may be NULL when ncontacts == 0). */
int idocp_model_from_urdf(const char* path_to_urdf, const int* contact_frames,
                          int ncontacts, idocp_model_t* out);

/* Parent joint (index into the model's joint arrays) and placement (R row-major, p) in that joint's frame of the frame with
 * pinocchio-compatible index frame_id: what Robot::framePlacement / getFrameJacobian (robot.hxx:166-188) are evaluated on. */
int idocp_model_frame_placement(const char* path_to_urdf, int frame_id, int* joint, double* R, double* p);
/* Frame name -> pinocchio-compatible frame index (robot.cpp printRobotModel
 * enumerates the same table); returns -1 if absent. */
int idocp_model_frame_id(const char* path_to_urdf, const char* frame_name);

/* World positions points[ncontacts][3] of the contact frames at configuration q:
 * Robot::updateFrameKinematics(q) + Robot::setContactPoints / getContactPoints
 * (include/idocp/robot/robot.hxx:85-91, 262-283).  Host arithmetic (problem
 * set-up before the contact sequence is built, examples/anymal/ocp_benchmark.cpp:
 * 104-106), not part of the hot path. */
int idocp_model_contact_positions(const idocp_model_t* model, const double* q, double* points);
/* Robot::framePosition / frameRotation / framePlacement (include/idocp/robot/robot.hxx:206-233) after updateFrameKinematics(q): world
 * placement of a frame that sits on `joint` with the local placement (R_local row-major [9], p_local [3]) -- the pair
 * idocp_model_frame_placement returns for a frame id of the URDF; joint -1 = fixed to the world.  Host arithmetic. */
int idocp_model_frame_world_placement(const idocp_model_t* model, const double* q, int joint, const double* R_local,
                                      const double* p_local, double* R_world, double* p_world);
/* Robot::integrateConfiguration / subtractConfiguration / normalizeConfiguration (include/idocp/robot/robot.hxx:96-147), host
 * arithmetic: q_out[nq] = q (+) length v (SE(3) exponential on a floating base); diff[nv] = q_plus (-) q_minus
 * (pinocchio::difference(q_minus, q_plus)); the base quaternion of q scaled to unit length.  What an MPC loop does between
 * two solver calls; the stage kernels carry their own copies of the same functions. */
int idocp_model_integrate_configuration(const idocp_model_t* model, const double* q, const double* v, double length,
                                        double* q_out);
int idocp_model_subtract_configuration(const idocp_model_t* model, const double* q_plus, const double* q_minus,
                                       double* diff);
int idocp_model_normalize_configuration(const idocp_model_t* model, double* q);

/* Guards against a driver compiled against an older header than the loaded library:
 * pass sizeof(idocp_model_t), sizeof(idocp_cost_t), sizeof(idocp_constraints_t);
 * returns IDOCP_E_ARG on a mismatch.  The C++ facade calls it from idocp::Robot. */
int idocp_abi_check(unsigned long model_size, unsigned long cost_size, unsigned long constraints_size);

void idocp_cost_init(idocp_cost_t* cost);                 /* all zero          */
void idocp_constraints_init(idocp_constraints_t* c);      /* reference defaults */

/* ---- UnOCPSolver (fixed-base, no contacts) ----------------------------- */

typedef struct idocp_unocp idocp_unocp_t;

/* UnOCPSolver::UnOCPSolver(robot, cost, constraints, T, N, nthreads)
 * (src/unocp/unocp_solver.cpp:11-48).  nthreads has no meaning on the GPU; it
 * is replaced by `batch` independent instances and a device ordinal.
 * The robot is a fixed-base serial chain of 2 .. 8 revolute joints (joint i the
 * child of joint i - 1, any axes); another model returns IDOCP_E_UNSUPPORTED and
 * idocp_last_error() names that range.  The same holds for idocp_unparnmpc_create,
 * idocp_unparnmpc_create_shard and idocp_rnea_derivatives. */
int idocp_unocp_create(const idocp_model_t* model, const idocp_cost_t* cost,
                       const idocp_constraints_t* constraints, double T, int N,
                       int batch, int device, idocp_unocp_t** out);
void idocp_unocp_destroy(idocp_unocp_t* h);
/* Deep copy of a UnOCPSolver / UnParNMPCSolver handle (the reference classes are copyable,
 * unocp_solver.hpp:59-62): same problem, same device, every device buffer and the line-search
 * filter copied. */
int idocp_unocp_clone(idocp_unocp_t* src, idocp_unocp_t** out);
/* Replace the cost of a UnOCPSolver / UnParNMPCSolver handle: the counterpart of idocp_ocp_set_cost.  The reference's
 * solvers share the CostFunction with the driver (unocp_solver.hpp: shared_ptr members), so references and weights changed
 * between two updateSolution calls take effect at the next one; here the cost is copied at creation and this call is how
 * an MPC loop moves its goal.  A task-space component cannot be added or removed (IDOCP_E_UNSUPPORTED). */
int idocp_unocp_set_cost(idocp_unocp_t* h, const idocp_cost_t* cost);

/* UnOCPSolver::setSolution(name, value) (unocp_solver.cpp:157-181): name in
 * {"q","v","a","u"}; value[dim] is written to every stage of every instance,
 * then the constraints are re-initialised. */
int idocp_unocp_set_solution(idocp_unocp_t* h, const char* name,
                             const double* value);
/* Same, one value per instance: values[batch][dim]. */
int idocp_unocp_set_solution_batch(idocp_unocp_t* h, const char* name,
                                   const double* values);
/* OCPSolver::setSolution / ParNMPCSolver::setSolution (ocp_solver.cpp:116-165, parnmpc_solver.cpp:128-180) write the
 * value and leave the slack / dual variables as they are (the driver calls initConstraints(t)): the setter behind the
 * facade's idocp::OCPSolver / idocp::ParNMPCSolver on a fixed-base robot without contacts, which are bound to these
 * kernels -- with no contact rows the two formulations condense one Newton system in two orders
 * (tests/test_oracle_fixed_base.py). */
int idocp_unocp_set_solution_only(idocp_unocp_t* h, const char* name, const double* value);
/* Per-stage reference poses of a TimeVaryingTaskSpace3DCost / TimeVaryingTaskSpace6DCost (cost.task_dim != 0): the values of
 * TimeVaryingTaskSpace6DRefBase::compute_q_6d_ref (time_varying_task_space_6d_cost.hpp:21-42) at t + i dt, i = 0 .. N.
 * refs: host, [N + 1][12] = rotation (row-major) then position; a 3D cost reads the position only.  Without a call the
 * constant cost.task_ref applies to every stage. */
int idocp_unocp_set_task_refs(idocp_unocp_t* h, const double* refs);
/* UnOCPSolver::initConstraints() (unocp_solver.cpp:59-70). */
int idocp_unocp_init_constraints(idocp_unocp_t* h);

/* UnOCPSolver::updateSolution(t, q, v, line_search) (unocp_solver.cpp:73-134).
 * q[batch][nq], v[batch][nv] are host pointers.  line_search != 0: filter line
 * search (unocp_solver.cpp:116-120), one filter per instance, see below. */
int idocp_unocp_update_solution(idocp_unocp_t* h, double t, const double* q,
                                const double* v, int line_search);
/* Same with q, v already resident in device memory (HBM); asynchronous on the
 * handle's stream -- call idocp_unocp_synchronize() before reading results. */
int idocp_unocp_update_solution_device(idocp_unocp_t* h, double t,
                                       const double* d_q, const double* d_v);
int idocp_unocp_synchronize(idocp_unocp_t* h);
/* Native stream handle (hipStream_t) so callers can record HIP events on it. */
void* idocp_unocp_stream(idocp_unocp_t* h);
/* Device allocation helpers for callers without a HIP binding (bench/tests). */
int idocp_device_alloc(void** d_ptr, unsigned long long nbytes);
int idocp_device_free(void* d_ptr);
int idocp_device_upload(void* d_dst, const void* h_src, unsigned long long nbytes);
/* Blocking copy back to the host (the results of the *_device entries); synchronize the handle first. */
int idocp_device_download(void* h_dst, const void* d_src, unsigned long long nbytes);
int idocp_device_count(int* count);

/* UnOCPSolver::computeKKTResidual(t, q, v) + KKTError() (unocp_solver.cpp:
 * 184-225): kkt_error[batch]. */
int idocp_unocp_compute_kkt_residual(idocp_unocp_t* h, double t, const double* q,
                                     const double* v);
int idocp_unocp_kkt_error(idocp_unocp_t* h, double* kkt_error);

/* UnOCPSolver::getSolution(name) (unocp_solver.cpp:240-309): name in
 * {"q","v","a","u","lmd","gmm","beta"}; out[(N+1)][dim] for one instance
 * (a, u, beta: N stages). */
int idocp_unocp_get_solution(idocp_unocp_t* h, const char* name, int instance,
                             double* out);
/* UnOCPSolver::getSolution(stage) (unocp_solver.hpp: `const SplitSolution& getSolution(int) const`):
 * the split solution of ONE stage in one device-to-host copy; out[7 nv] = lmd gmm q v a u beta
 * (a, u, beta are meaningless on the terminal stage N). */
int idocp_unocp_get_split_solution(idocp_unocp_t* h, int instance, int stage, double* out);
/* Newton direction of the last updateSolution (parity tests): name in
 * {"dq","dv","da","du","dlmd","dgmm","dbeta"}; same shapes. */
int idocp_unocp_get_direction(idocp_unocp_t* h, const char* name, int instance,
                              double* out);
/* Step sizes of the last updateSolution: primal[batch], dual[batch]. */
int idocp_unocp_get_step_sizes(idocp_unocp_t* h, double* primal, double* dual);
/* Riccati factorization of one instance: P[N+1][2nv*2nv] (col-major, blocks
 * [Pqq Pqv; Pvq Pvv]), s[N+1][2nv], K[N][nv*2nv] (col-major), k[N][nv]. Any
 * pointer may be NULL.  (split_riccati_factorization.hpp:15-134,
 * lqr_state_feedback_policy.hpp:11-28) */
int idocp_unocp_get_riccati(idocp_unocp_t* h, int instance, double* P, double* s,
                            double* K, double* k);
/* OCPSolver::getStateFeedbackGain (ocp_solver.cpp:101-111) on the fixed-base robot without contacts: the TORQUE policy
 * du = Kq dq + Kv dv, i.e. the acceleration policy above mapped through the linearised inverse dynamics of the same
 * linearisation (unconstrained_dynamics.hxx:84-92): Kq = dID/dq + M Ka_q, Kv = dID/dv + M Ka_v; nv x nv col-major. */
int idocp_unocp_get_torque_feedback_gain(idocp_unocp_t* h, int instance, int stage,
                                         double* Kq, double* Kv);
/* Slack / dual variables of the IPM, [N][dimc] for one instance. */
int idocp_unocp_get_constraint_data(idocp_unocp_t* h, int instance,
                                    double* slack, double* dual);
int idocp_unocp_dimc(const idocp_unocp_t* h);
/* UnOCPSolver::isCurrentSolutionFeasible (unocp_solver.cpp:228-237): feasible[batch]
 * = 1 if the primal iterate satisfies the joint limits on every stage (with the
 * time-step gating of constraints_data.hpp:18-42), else 0; where[batch] (may be
 * NULL) = first offending stage or -1. */
int idocp_unocp_is_current_solution_feasible(idocp_unocp_t* h, int* feasible, int* where);

/* Filter line search of the two fixed-base solvers (UnLineSearch, include/idocp/line_search/unline_search.hpp:62-92;
 * LineSearchFilter, src/line_search/line_search_filter.cpp): idocp_unocp_update_solution / idocp_unparnmpc_update_solution
 * with line_search != 0 evaluate the trial iterates on the device and keep one filter per instance.
 * UnOCPSolver / UnParNMPCSolver::clearLineSearchFilter: */
int idocp_unocp_clear_line_search_filter(idocp_unocp_t* h);
/* UnLineSearch::computeCostAndViolation of s + alpha[b] d for every instance (alpha = 0: the iterate itself), with the
 * measured state of the last host-pointer update / residual call: cost[batch], violation[batch]. */
int idocp_unocp_line_search_eval(idocp_unocp_t* h, const double* alpha, double* cost,
                                 double* violation);

/* ---- UnParNMPCSolver (include/idocp/unocp/unparnmpc_solver.hpp:31-189, src/unocp/unparnmpc_solver.cpp) ----
 * The stage-parallel solver of the fixed-base problem: N backward-Euler stages (stage i at t + (i+1) dt, created with
 * constraint time step i + 1, the last one terminal), per-stage KKT inverse, coarse update and the four correction
 * sweeps of UnBackwardCorrection (src/unocp/unbackward_correction.cpp:55-132).  The handle type is shared with
 * UnOCPSolver: idocp_unocp_set_solution[_batch], _init_constraints, _get_solution, _get_direction, _get_step_sizes,
 * _kkt_error, _get_constraint_data, _is_current_solution_feasible, _synchronize, _stream and _destroy work on it (the
 * stage-wise getters return the N stages in their first N rows); the entry points below replace the rest. */
int idocp_unparnmpc_create(const idocp_model_t* model, const idocp_cost_t* cost,
                           const idocp_constraints_t* constraints, double T, int N, int batch,
                           int device, idocp_unocp_t** out);
/* UnParNMPCSolver::initBackwardCorrection (unparnmpc_solver.cpp:69-71) */
int idocp_unparnmpc_init_backward_correction(idocp_unocp_t* h, double t);
/* UnParNMPCSolver::updateSolution (unparnmpc_solver.cpp:74-103); q, v: [batch][nv] on the host */
int idocp_unparnmpc_update_solution(idocp_unocp_t* h, double t, const double* q, const double* v,
                                    int line_search);
/* the same with device-resident (q, v), asynchronous on the handle's stream */
int idocp_unparnmpc_update_solution_device(idocp_unocp_t* h, double t, const double* d_q,
                                           const double* d_v);
/* UnParNMPCSolver::computeKKTResidual (unparnmpc_solver.cpp:169-187); read it with idocp_unocp_kkt_error */
int idocp_unparnmpc_compute_kkt_residual(idocp_unocp_t* h, double t, const double* q,
                                         const double* v);
/* One phase of updateSolution (parity tests, roofline measurement): 0 linearize, 1 KKT inverse + coarse update,
 * 2 backward serial, 3 backward parallel, 4 forward serial, 5 forward parallel + direction + step sizes, 6 integrate. */
int idocp_unparnmpc_launch_phase(idocp_unocp_t* h, int phase, const double* d_q, const double* d_v);
/* The coarse / corrected iterate s_new of the backward correction (fields lmd, gmm, a, q, v), like
 * idocp_unocp_get_solution. */
int idocp_unparnmpc_get_new_solution(idocp_unocp_t* h, const char* name, int instance, double* out);

/* Horizon sharding of UnParNMPCSolver (the fixed-base twin of idocp_parnmpc_create_shard; protocol and halo kinds as in
 * idocp_amd/parnmpc_dist.py): the handle holds the stages [stage_begin, stage_end) of a horizon of N stages over T.
 * Halo kinds: 0 state_last (q, v of the last stage -> the right neighbour's previous state), 1 costate_first (lmd, gmm of the
 * first stage -> left), 2 aux_first (aux_mat of the first stage -> left), 3 bwd_first (corrected lmd, gmm of the first stage
 * -> left, pipeline of the backward serial sweep), 4 fwd_last (corrected q, v of the last stage -> right, pipeline of the
 * forward serial sweep).  Buffers are device pointers, [batch][idocp_unparnmpc_halo_size(kind)]. */
int idocp_unparnmpc_create_shard(const idocp_model_t* model, const idocp_cost_t* cost,
                                 const idocp_constraints_t* constraints, double T, int N, int stage_begin,
                                 int stage_end, int batch, int device, idocp_unocp_t** out);
int idocp_unparnmpc_halo_size(int kind);      /* sizes of a 7-joint chain (iiwa14) */
int idocp_unparnmpc_halo_size_of(const idocp_unocp_t* h, int kind);      /* sizes of the handle's chain: 2 nv, or (2 nv)^2 for kind 2 */
int idocp_unparnmpc_export_halo(idocp_unocp_t* h, int kind, double* d_buf);
int idocp_unparnmpc_import_halo(idocp_unocp_t* h, int kind, const double* d_buf);
/* device buffers of the previous state (rank 0: the measured state) and of the (primal, dual) step sizes [batch][2] */
int idocp_unparnmpc_prev_state(idocp_unocp_t* h, double** d_q, double** d_v);
int idocp_unparnmpc_step_sizes_device(idocp_unocp_t* h, double** d_steps);
/* squared KKT error of the local stages, d_err2[batch] on the device (to be summed over the ranks) */
int idocp_unparnmpc_kkt_error_squared_device(idocp_unocp_t* h, double t, double* d_err2);

/* Kernel-level entry points used by the parity tests and the roofline
 * measurement (one launch each, on the handle's stream). */
int idocp_unocp_launch_linearize(idocp_unocp_t* h, double t, const double* d_q,
                                 const double* d_v);
int idocp_unocp_launch_riccati(idocp_unocp_t* h, const double* d_q,
                               const double* d_v);
int idocp_unocp_launch_expand(idocp_unocp_t* h);
int idocp_unocp_launch_integrate(idocp_unocp_t* h);
/* One single kernel launch, for per-kernel timing: kernel_id 0 = K1 linearize,
 * 1 = S1 backward Riccati, 2 = S2 forward Riccati, 3 = K2 expand, 4 = step-size
 * reduction, 5 = K3 integrate. */
int idocp_unocp_launch_kernel(idocp_unocp_t* h, int kernel_id, const double* d_q,
                              const double* d_v);
/* Inverse dynamics + its derivatives for `n` independent samples on the device
 * (Robot::RNEA / RNEADerivatives, include/idocp/robot/robot.hxx:444-500).
 * q[n][nq], v[n][nv], a[n][nv] host; tau[n][nv]; dq/dv/da[n][nv*nv] col-major.
 * model: a fixed-base serial chain of 2 .. 8 revolute joints. */
int idocp_rnea_derivatives(const idocp_model_t* model, int n, const double* q,
                           const double* v, const double* a, double* tau,
                           double* dtau_dq, double* dtau_dv, double* dtau_da,
                           int device);

/* ---- OCPSolver (floating base + point contacts) --------------------------- */

typedef struct idocp_ocp idocp_ocp_t;

/* OCPSolver::OCPSolver(robot, cost, constraints, T, N, max_num_impulse, nthreads)
 * (src/ocp/ocp_solver.cpp:9-47).  This build carries the kernels for a quadruped
 * (free-flyer + 4 legs x 3 revolute joints, one point contact per foot) and a
 * contact sequence WITHOUT discrete events (setContactStatusUniformly only);
 * created this way it holds event-free horizons only (max_num_impulse = 0). */
int idocp_ocp_create(const idocp_model_t* model, const idocp_cost_t* cost,
                     const idocp_constraints_t* constraints, double T, int N,
                     int batch, int device, idocp_ocp_t** out);
/* OCPSolver(robot, cost, constraints, T, N, max_num_impulse, nthreads) (ocp_solver.cpp:10-47):
 * reserves stages for up to max_num_impulse discrete events (impulse + aux stage or a
 * lift stage each) so that contact sequences can be pushed. */
int idocp_ocp_create_hybrid(const idocp_model_t* model, const idocp_cost_t* cost,
                            const idocp_constraints_t* constraints, double T, int N,
                            int max_num_impulse, int batch, int device, idocp_ocp_t** out);
void idocp_ocp_destroy(idocp_ocp_t* h);
/* OCPSolver::setContactStatusUniformly (ocp_solver.cpp:169-171): active[ncontacts]
 * flags and the world contact points contact_points[ncontacts][3]
 * (ContactStatus::setContactPoints). */
int idocp_ocp_set_contact_status_uniformly(idocp_ocp_t* h, const int* active,
                                           const double* contact_points);
/* OCPSolver::pushBackContactStatus / setContactPoints / popBackContactStatus /
 * popFrontContactStatus (ocp_solver.cpp:174-197) -> ContactSequence (include/idocp/hybrid/
 * contact_sequence.hxx:52-268) and DiscreteEvent (discrete_event.hxx:57-84): a status
 * that activates a contact is an impulse event (impulse + aux stage and a switching
 * constraint two stages ahead), one that only deactivates contacts is a lift event. */
int idocp_ocp_push_back_contact_status(idocp_ocp_t* h, const int* active,
                                       const double* contact_points, double switching_time);
int idocp_ocp_set_contact_points(idocp_ocp_t* h, int contact_phase, const double* contact_points);
int idocp_ocp_pop_back_contact_status(idocp_ocp_t* h);
int idocp_ocp_pop_front_contact_status(idocp_ocp_t* h);
/* The stages in time order after OCPDiscretizer::discretizeOCP(contact_sequence, t)
 * (include/idocp/hybrid/ocp_discretizer.hxx:65-374).  Returns the chain length
 * M = N + 1 + 2 N_impulse + N_lift (or a negative error code); arrays of `capacity`
 * entries, any may be NULL: kind (0 stage, 1 impulse, 2 aux, 3 lift, 4 terminal), index
 * (grid stage / impulse index / lift index), storage slot, time step, dimf, rows of the
 * switching constraint carried by the stage. */
/* Warm start along the chain of the current discretisation (event stages included): values[M][dim] in the order of
 * idocp_ocp_get_chain, written to every instance.  (The grid-stage setters idocp_ocp_set_solution_stages /
 * idocp_parnmpc_set_aux_mat cannot reach the impulse / aux / lift slots; this is what an MPC loop that shifts a solution with
 * discrete events along the horizon needs -- the reference does it through the public members of its Solution container.) */
int idocp_ocp_set_solution_chain(idocp_ocp_t* h, const char* name, int M, const double* values);
int idocp_parnmpc_set_aux_mat_chain(idocp_ocp_t* h, int M, const double* values);
/* ... and its counterpart: aux_mat of every stage of the chain of one instance, out[M][nx * nx] (column-major per stage).  With
 * idocp_ocp_get_solution_chain this carries a converged ParNMPC solver over into another handle (another batch size, a shard). */
int idocp_parnmpc_get_aux_mat_chain(idocp_ocp_t* h, int instance, double* out);
/* The coarse / corrected iterate s_new of the backward correction along the chain (SplitBackwardCorrection::s_new_,
 * split_backward_correction.hxx:50-82; after idocp_parnmpc_launch_phase 0 - 2 the coarse update, after the correction phases the corrected
 * iterate).  name: lmd gmm u q v xi; on an impulse stage "u" holds the impulse forces f and "xi" the multipliers mu of the velocity
 * constraint, both packed (active contacts first); "xi" of an aux stage is its switching multiplier.  out[M][dim], dim = nv, nv, nu, nq,
 * nv, 3 * max_point_contacts. */
int idocp_parnmpc_get_new_solution_chain(idocp_ocp_t* h, const char* name, int instance, double* out);
int idocp_ocp_get_chain(idocp_ocp_t* h, double t, int capacity, int* kind, int* index, int* slot,
                        double* dt, int* dimf, int* sw_dimi);
/* TimeVaryingTaskSpace3DCost / TimeVaryingTaskSpace6DCost on a floating-base robot (src/cost/time_varying_task_space_3d_cost.cpp,
 * time_varying_task_space_6d_cost.cpp: the reference object is asked for its pose at the time of every stage).  The device cannot call the
 * caller's reference object, so the poses are evaluated up front: idocp_ocp_get_chain_times lists the times of the M stages of the chain
 * discretised at t (the order of idocp_ocp_get_chain: grid stages at t + i dt, impulse / aux / lift stages at their event times, the
 * terminal stage at t + T; returns M), idocp_ocp_set_task_refs hands the M poses over, refs[M][12] = rotation (row-major, 9; identity for
 * the 3D cost) then position (3).  They apply to every call with this t; a call with another t, or a chain of another length, fails with
 * IDOCP_E_ARG until new poses are set.  cost.task_time_varying must be set at creation (OCPSolver and ParNMPCSolver on any chain,
 * discrete events included -- as for the constant-reference costs). */
int idocp_ocp_get_chain_times(idocp_ocp_t* h, double t, int capacity, double* times);
int idocp_ocp_set_task_refs(idocp_ocp_t* h, double t, int M, const double* refs);
/* OCPSolver::setSolution (ocp_solver.cpp:95-165): name in {"q","v","a","f","u"};
 * "f" takes one 3-vector written to every contact.  Does not re-initialise the
 * constraints (like the reference). */
int idocp_ocp_set_solution(idocp_ocp_t* h, const char* name, const double* value);
int idocp_ocp_set_solution_batch(idocp_ocp_t* h, const char* name, const double* values);
/* Warm start (an MPC loop keeps the iterate of the previous sampling instant; the reference does so implicitly because the solver
 * object lives on): one field of every grid stage, values[nstages][dim], the same for all instances.  name: q v a u beta f mu
 * (dim 3 * max contacts) lmd gmm nu_passive; nstages <= N + 1 for lmd gmm q v of an OCPSolver, <= N otherwise. */
int idocp_ocp_set_solution_stages(idocp_ocp_t* h, const char* name, int nstages, const double* values);
/* OCPSolver::initConstraints(t) (ocp_solver.cpp:60-64). */
int idocp_ocp_init_constraints(idocp_ocp_t* h, double t);
/* OCPSolver::updateSolution (ocp_solver.cpp:67-92). q[batch][nq], v[batch][nv].  line_search != 0: the filter line search of
 * src/line_search/line_search.cpp on the primal step (one filter per instance; cost and l1 constraint violation of the trial
 * iterates are evaluated on the device, the filter logic runs on the host). */
int idocp_ocp_update_solution(idocp_ocp_t* h, double t, const double* q,
                              const double* v, int line_search);
int idocp_ocp_update_solution_device(idocp_ocp_t* h, double t, const double* d_q,
                                     const double* d_v);
/* OCPSolver::clearLineSearchFilter (ocp_solver.cpp:196-199). */
int idocp_ocp_clear_line_search_filter(idocp_ocp_t* h);
/* Probing the line search (tests): the Newton direction and step sizes of the current iterate WITHOUT integrating, then
 * LineSearch::computeCostAndViolation of s (+) alpha[b] d per instance (alpha = 0: the iterate itself). */
int idocp_ocp_compute_direction(idocp_ocp_t* h, double t, const double* q, const double* v);
int idocp_ocp_line_search_eval(idocp_ocp_t* h, const double* alpha, double* cost, double* violation);
/* The same iteration submitted as ONE hipGraph launch (captured on first use, re-captured when the discretisation or the input
 * buffers change): the latency mode of the solver -- at batch 1 the launches, not the kernels, set the pace. */
int idocp_ocp_update_solution_graph(idocp_ocp_t* h, double t, const double* d_q,
                                    const double* d_v);
int idocp_ocp_synchronize(idocp_ocp_t* h);
void* idocp_ocp_stream(idocp_ocp_t* h);
/* OCPSolver::computeKKTResidual + KKTError (ocp_solver.cpp:202-213). */
int idocp_ocp_compute_kkt_residual(idocp_ocp_t* h, double t, const double* q,
                                   const double* v);
int idocp_ocp_kkt_error(idocp_ocp_t* h, double* kkt_error);
/* OCPSolver::getSolution(name): q v a u f lmd gmm beta mu nu_passive; out[(N+1)][dim]
 * (f, mu: [ncontacts*3] per stage; stage-only fields fill N rows). */
int idocp_ocp_get_solution(idocp_ocp_t* h, const char* name, int instance, double* out);
/* OCPSolver::getSolution(stage) (ocp_solver.hpp:97) / ParNMPCSolver::getSolution(stage): the split
 * solution of ONE grid stage in one device-to-host copy -- the call an MPC loop makes every cycle.
 * out[3 nv + nq + nv + nu + nv + 2 * 3 ncontacts + 6] = lmd gmm q v a u beta f mu nu_passive
 * (split_solution.hxx:10-31); only lmd gmm q v are meaningful on the terminal stage. */
int idocp_ocp_get_split_solution(idocp_ocp_t* h, int instance, int stage, double* out);
/* The contact status grid stage `stage` of the current discretisation is linearised with
 * (SplitSolution::setContactStatus / isContactActive / dimf, split_solution.hxx:41-57): active[ncontacts]
 * flags; returns dimf (3 per active contact; 0 on the terminal stage) or a negative error code.  It sizes
 * SplitSolution::f_stack() / mu_stack() (split_solution.hpp:93-122) in the facade's getSolution(stage). */
int idocp_ocp_get_stage_contact_status(idocp_ocp_t* h, int stage, int* active);
/* Newton direction: dq dv da du df dlmd dgmm dbeta dmu dnu_passive dxi.  df / dmu are [ncontacts][3] per stage with zeros for the
 * contacts that are not active there, dxi has zeros behind the stage's switching-constraint rows (SplitDirection::df / dmu / dxi only
 * have the active rows, split_direction.hxx:150-229). */
int idocp_ocp_get_direction(idocp_ocp_t* h, const char* name, int instance, double* out);
/* The same fields for every stage of the chain (incl. impulse / aux / lift stages), in
 * chain order: out[M][dim].  Extra names: "xi" / "dxi" (multiplier of the switching
 * constraint, max_dimf entries).  On impulse stages "a" / "da" hold dv / ddv. */
int idocp_ocp_get_solution_chain(idocp_ocp_t* h, const char* name, int instance, double* out);
int idocp_ocp_get_direction_chain(idocp_ocp_t* h, const char* name, int instance, double* out);
int idocp_ocp_get_step_sizes(idocp_ocp_t* h, double* primal, double* dual);
/* P[N+1][2nv*2nv], s[N+1][2nv], K[N][nu*2nv] (nu x 2nv col-major), k[N][nu]. */
int idocp_ocp_get_riccati(idocp_ocp_t* h, int instance, double* P, double* s, double* K,
                          double* k);
/* Chain order: P[M][..], s[M][..], K[M-1][..], k[M-1][..]. */
int idocp_ocp_get_riccati_chain(idocp_ocp_t* h, int instance, double* P, double* s, double* K,
                                double* k);
/* OCPSolver::getStateFeedbackGain (ocp_solver.cpp:101-111): Kq, Kv (nu x nv col-major). */
int idocp_ocp_get_state_feedback_gain(idocp_ocp_t* h, int instance, int stage, double* Kq,
                                      double* Kv);
int idocp_ocp_dimc(const idocp_ocp_t* h);
/* OCPSolver::isCurrentSolutionFeasible (ocp_solver.cpp:216-248) and
 * ParNMPCSolver::isCurrentSolutionFeasible (parnmpc_solver.cpp:231-273): feasible[batch]
 * = 1 if the primal iterate satisfies the joint limits and the linearised (impulse)
 * friction cones on every stage of the current chain; where[batch] (may be NULL) =
 * chain position of the first offending stage (stages, then impulses, aux, lifts) or -1. */
int idocp_ocp_is_current_solution_feasible(idocp_ocp_t* h, int* feasible, int* where);
int idocp_ocp_get_constraint_data(idocp_ocp_t* h, int instance, double* slack, double* dual);
/* Condensed LQR data of one stage after the linearisation kernels (parity tests):
 * Qxx[2nv*2nv], Qxu[2nv*nu], Quu[nu*nu], A[2nv*2nv], B[2nv*nu], lx[2nv], lu[nu], Fx[2nv]. */
/* The inverse of idocp_ocp_get_lqr_stage, for every instance of the handle: writes the condensed LQR stage the backward Riccati sweep reads
 * (SplitKKTMatrix / SplitKKTResidual after condensation, split_kkt_matrix.hxx, split_kkt_residual.hxx).  Blocks column-major: Qxx [2nv x 2nv], Qxu
 * [2nv x nu], Quu [nu x nu], Fqq6 / Fqv6 [6 x 6] (the base blocks of Fqq, Fqv), Fvq, Fvv [nv x nv], Fvu [nv x nu], lx [2nv], lu [nu], Fx [2nv];
 * terminal != 0: Qxx and lx only.  For tests that run the sweep alone (idocp_ocp_launch_kernel id 2) on a problem with a known answer. */
int idocp_ocp_set_lqr_stage(idocp_ocp_t* h, int stage, int terminal, const double* Qxx, const double* Qxu, const double* Quu,
                            const double* Fqq6, const double* Fqv6, const double* Fvq, const double* Fvv, const double* Fvu,
                            const double* lx, const double* lu, const double* Fx);
/* For tests: the same blocks by position in the chain of the current discretisation (grid, impulse, aux, lift and terminal nodes), of one
 * instance or, with instance == -1, of all.  The node's kind decides what is read: a terminal node takes Qxx and lx only; an impulse node has no
 * control -- its record gets what the condensation leaves there (Quu = I, Qxu = 0, Fvu = 0, lu = 0, Fqv6 = 0) and Qxu, Quu, Fqv6, Fvu, lu may be
 * NULL.  idocp_ocp_set_lqr_stage is this entry on a grid stage for all instances.  IDOCP_E_ARG, with a text that begins with the entry's name,
 * for a ParNMPC handle and an instance or position out of range. */
int idocp_ocp_set_lqr_stage_chain(idocp_ocp_t* h, int instance, int position, const double* Qxx, const double* Qxu, const double* Quu,
                                  const double* Fqq6, const double* Fqv6, const double* Fvq, const double* Fvv, const double* Fvu,
                                  const double* lx, const double* lu, const double* Fx);
/* For tests: the switching constraint Phix dx + Phiu du + P = 0 carried by one chain position, as the backward sweep reads it: P [dimi],
 * Phix [dimi x 2nv], Phiu [dimi x nu], column-major with leading dimension dimi; of one instance or, with instance == -1, of all.  Rows
 * dimi .. max_dimf - 1 of the record stay as they are: the kernels that fill it write rows 0 .. dimi - 1 only.  IDOCP_E_ARG, with a text that
 * begins with the entry's name, for a ParNMPC handle, a position out of range, a position without a switching constraint, and a dimi that is
 * not the node's (idocp_ocp_get_chain: sw_dimi). */
int idocp_ocp_set_switching_constraint(idocp_ocp_t* h, int instance, int position, int dimi, const double* P, const double* Phix,
                                       const double* Phiu);
/* For tests: the multiplier policy dxi = M dx + m the backward sweep left at one chain position (SplitConstrainedRiccatiFactorization,
 * split_riccati_factorizer.hxx:71-74): M [dimi x 2nv] column-major with leading dimension dimi, m [dimi]; either may be NULL.  Returns dimi, or
 * IDOCP_E_ARG with a text as above. */
int idocp_ocp_get_switching_policy(idocp_ocp_t* h, int instance, int position, double* M, double* m);
/* ContactDynamicsData of a grid stage after the condensation (include/idocp/ocp/contact_dynamics_data.hxx:8-29): MJtJinv [n * n], MJtJinv_dIDCdqv
 * [n * 2 nv], MJtJinv_IDC [n], dense column-major with n = nv + dimf rows (the rows of the active contacts packed).  Returns dimf (>= 0) or an
 * error code (< 0).  For tests: M, J and the derivatives of [ID; C] follow from the three by one inverse. */
int idocp_ocp_get_contact_dynamics(idocp_ocp_t* h, int instance, int stage, double* MJtJinv, double* MJtJinv_dIDCdqv,
                                   double* MJtJinv_IDC);
/* The same by position in the chain of the current discretisation: grid, aux, lift and IMPULSE stages (there: ImpulseDynamicsForwardEulerData,
 * include/idocp/impulse/impulse_dynamics_forward_euler_data.hxx -- MJtJinv over the impulse's contacts, the blocks of [ImD; V] in place of [ID; C]). */
int idocp_ocp_get_contact_dynamics_chain(idocp_ocp_t* h, int instance, int position, double* MJtJinv, double* MJtJinv_dIDCdqv,
                                         double* MJtJinv_IDC);
/* For tests: the terms of one chain position that carry frame Jacobians of their own (ContactDistance rows, TaskSpace3DCost / TaskSpace6DCost
 * components), as the last linearisation left them BEFORE they were added into the stage -- any node kind, ParNMPC's last stage included.
 * With nc = max_point_contacts, nt = 1 + IDOCP_MAX_EXTRA_TASKS, every array nullable: z[nc] world heights of the contact frames,
 * Jc[nc][nv] the ContactDistance rows (zero on an active contact), w[nc] their Hessian weights, JJ[nt * 6][nv] the task rows (six per component,
 * the last three zero for a 3D one; unused components zero), tw[nt * 6] their Hessian weights, lq[nv] the share of the gradient, and the scalars
 * cost, violation, kkt_error of the stage's share.  IDOCP_E_ARG (with a text) for a handle without such terms, an instance or position
 * out of range, and the placeholder behind ParNMPC's last stage.  One device-to-host copy; launches nothing. */
int idocp_ocp_get_ext_terms(idocp_ocp_t* h, int instance, int position, double* z, double* Jc, double* w, double* JJ, double* tw, double* lq,
                            double* cost, double* violation, double* kkt_error);
int idocp_ocp_get_lqr_stage(idocp_ocp_t* h, int instance, int stage, double* Qxx, double* Qxu,
                            double* Quu, double* A, double* B, double* lx, double* lu,
                            double* Fx);
/* Diagnostic: wall-clock stamps (100 MHz ticks) taken at the phase boundaries of one
 * workgroup of the condensation kernel during the last launch; n <= 64. */
int idocp_ocp_get_profile(idocp_ocp_t* h, long long* out, int n);
/* ---- ParNMPCSolver (src/ocp/parnmpc_solver.cpp), horizons without discrete events -------------
 * Backward-Euler stages + backward correction (stage-parallel Newton) instead of the Riccati
 * sweep.  The handle is an idocp_ocp_t: contact status, setSolution, initConstraints, KKTError,
 * getters and step sizes go through the idocp_ocp_* entry points above with N stages 0..N-1
 * (stage i lives at t + (i+1) T/N; stage N-1 carries the terminal cost). */
int idocp_parnmpc_create(const idocp_model_t* model, const idocp_cost_t* cost,
                         const idocp_constraints_t* constraints, double T, int N, int batch,
                         int device, idocp_ocp_t** out);
/* ParNMPCSolver(robot, cost, constraints, T, N, max_num_impulse, nthreads) (include/idocp/ocp/parnmpc_solver.hpp) for horizons
 * with discrete events: idocp_ocp_push_back_contact_status / set_contact_points / pop_* act on the handle as for OCPSolver;
 * the chain of stages (idocp_ocp_get_chain) follows ParNMPCDiscretizer (aux / impulse / lift stages in FRONT of the grid stage
 * that follows the event). */
int idocp_parnmpc_create_hybrid(const idocp_model_t* model, const idocp_cost_t* cost,
                                const idocp_constraints_t* constraints, double T, int N, int max_num_impulse,
                                int batch, int device, idocp_ocp_t** out);
/* ParNMPCSolver::initBackwardCorrection (parnmpc_solver.cpp:66-70): aux_mat of every stage
 * = terminal cost Hessian. */
int idocp_parnmpc_init_backward_correction(idocp_ocp_t* h, double t);
/* Warm start of the correction state: BackwardCorrectionSolver::aux_mat_ of stages 0 .. nstages - 1, values[nstages][nx * nx]
 * column-major (what initBackwardCorrection fills with the terminal cost Hessian, backward_correction_solver.cpp:62-80). */
int idocp_parnmpc_set_aux_mat(idocp_ocp_t* h, int nstages, const double* values);
/* ParNMPCSolver::updateSolution (parnmpc_solver.cpp:73-103): coarseUpdate,
 * backwardCorrectionSerial / Parallel, forwardCorrectionSerial / Parallel, step sizes,
 * integrateSolution.  q[batch][nq], v[batch][nv]; line_search != 0: the filter line search on the primal step
 * (LineSearch::computeStepSize for ParNMPC, src/line_search/line_search.cpp:199-301) on a handle that holds the whole horizon,
 * discrete events included; on a shard of a horizon IDOCP_E_UNSUPPORTED -- the sharded driver's
 * idocp_parnmpc_dist_update_solution_ls evaluates every probe collectively (its hooks are installed for the duration of that call only).  idocp_ocp_line_search_eval / idocp_ocp_clear_line_search_filter
 * work on ParNMPC handles as well. */
int idocp_parnmpc_update_solution(idocp_ocp_t* h, double t, const double* q, const double* v,
                                  int line_search);
/* The same up to and including the step sizes, without integrating (the state idocp_ocp_line_search_eval probes). */
int idocp_parnmpc_compute_direction(idocp_ocp_t* h, double t, const double* q, const double* v);
int idocp_parnmpc_update_solution_device(idocp_ocp_t* h, double t, const double* d_q,
                                         const double* d_v);
/* One phase of updateSolution (bench / tests): 0 tangent RNEA, 1 backward-Euler condensation,
 * 2 KKT inverse + coarse update, 3 backward serial, 4 backward parallel, 5 forward serial,
 * 6 forward parallel + direction, 7 expansion + step sizes, 8 step-size reduction,
 * 9 dual expansion + integration. */
int idocp_parnmpc_launch_phase(idocp_ocp_t* h, int phase, const double* d_q, const double* d_v);
/* ParNMPCSolver::computeKKTResidual (parnmpc_solver.cpp:200-206); read with idocp_ocp_kkt_error. */
int idocp_parnmpc_compute_kkt_residual(idocp_ocp_t* h, double t, const double* q, const double* v);
/* Horizon sharding (BASELINE.json configs[3]; protocol in idocp_amd/parnmpc_dist.py): one handle per
 * process holds the stages [stage_offset, stage_offset + N) of a longer horizon (T = N * dt of the
 * shard).  Halos are packed into / unpacked from caller-owned DEVICE buffers d_buf[batch][size] that
 * the caller moves between ranks (RCCL send / recv); kinds: 0 state_last (q, v -> right),
 * 1 costate_first (lmd, gmm, q -> left), 2 aux_first (-> left), 3 bwd_first (corrected lmd, gmm ->
 * left), 4 fwd_last (corrected q, v -> right), 5 aux_all (initBackwardCorrection broadcast). */
int idocp_parnmpc_create_shard(const idocp_model_t* model, const idocp_cost_t* cost,
                               const idocp_constraints_t* constraints, double T, int N,
                               int stage_offset, int has_terminal, int has_prev, int batch,
                               int device, idocp_ocp_t** out);
/* The same for a horizon WITH discrete events: every rank creates its handle with the whole horizon (T, N, max_num_impulse) and
 * pushes the whole contact sequence; the handle keeps the grid stages [stage_begin, stage_end) of the ParNMPCDiscretizer chain
 * and the event stages in front of each of them.  Halos as above. */
int idocp_parnmpc_create_hybrid_shard(const idocp_model_t* model, const idocp_cost_t* cost,
                                      const idocp_constraints_t* constraints, double T, int N, int max_num_impulse,
                                      int stage_begin, int stage_end, int batch, int device, idocp_ocp_t** out);
int idocp_parnmpc_halo_size(int kind);
int idocp_parnmpc_export_halo(idocp_ocp_t* h, int kind, double* d_buf);
int idocp_parnmpc_import_halo(idocp_ocp_t* h, int kind, const double* d_buf);
/* The same pack / unpack kernels enqueued on the handle's stream WITHOUT the host waiting for them: for a
 * stream-ordered transport (the C++ driver below: pack -> ncclSend, ncclRecv -> unpack on one stream). */
int idocp_parnmpc_export_halo_async(idocp_ocp_t* h, int kind, double* d_buf);
int idocp_parnmpc_import_halo_async(idocp_ocp_t* h, int kind, const double* d_buf);
/* ---- multi-GPU driver of the sharded horizon, in C++ over RCCL (idocp_amd/csrc/parnmpc_dist.hip) ------------------------
 * Counterpart of BackwardCorrectionSolver (src/ocp/backward_correction_solver.cpp:255-366) for one process per GPU: every rank
 * creates its shard (idocp_parnmpc_create_shard / _create_hybrid_shard), a communicator, attaches one to the other and then calls
 * the idocp_parnmpc_dist_* entry points collectively.  The halo exchange (point-to-point ncclSend / ncclRecv with the two
 * neighbours, all-reduce of step sizes and KKT error) is enqueued on the shard's stream between its kernels; nothing in an
 * iteration synchronises with the host.  The unique id is made on rank 0 and distributed by the caller (MPI, a file, a store). */
#define IDOCP_COMM_ID_BYTES 128
typedef struct idocp_comm idocp_comm_t;
int idocp_comm_get_unique_id(void* id /* IDOCP_COMM_ID_BYTES */);
int idocp_comm_init_rank(const void* id, int rank, int world, int device, idocp_comm_t** out);
/* `world` endpoints on ONE GPU in one process (out[world]; one host thread per endpoint): the transport of the single-GPU test
 * of this driver, not a product path. */
int idocp_comm_init_local(int world, int device, idocp_comm_t** out);
/* Host-staged transport through caller-supplied functions (an MPI or gloo communicator the caller already owns; the cross-process test of
 * the driver on a one-GPU box).  The driver makes the SAME calls in the same order and grouping as on RCCL
 * (src/ocp/backward_correction_solver.cpp:255-366 is the computation being distributed):
 *   send / recv   n doubles to / from rank `peer`.  in_group != 0: between group_start and group_end the call may only POST the transfer
 *                 (buffers stay valid until group_end returns; ncclGroupStart / ncclGroupEnd semantics: a send and its matching receive of the
 *                 same group never block each other); in_group == 0: complete before returning
 *   group_start / group_end   optional (NULL: every send / recv must then be able to complete on its own)
 *   allreduce     in place on n doubles, op 0 = sum, 1 = min;   broadcast   n doubles from rank `root`
 *   destroy       optional, called by idocp_comm_destroy
 * Every function returns 0 on success. */
typedef struct idocp_comm_callbacks {
  void* ctx;
  int (*send)(void* ctx, const double* buf, unsigned long n, int peer, int in_group);
  int (*recv)(void* ctx, double* buf, unsigned long n, int peer, int in_group);
  int (*group_start)(void* ctx);
  int (*group_end)(void* ctx);
  int (*allreduce)(void* ctx, double* buf, unsigned long n, int op);
  int (*broadcast)(void* ctx, double* buf, unsigned long n, int root);
  void (*destroy)(void* ctx);
} idocp_comm_callbacks_t;
int idocp_comm_init_callbacks(int rank, int world, int device, const idocp_comm_callbacks_t* cb, idocp_comm_t** out);
void idocp_comm_destroy(idocp_comm_t* c);
int idocp_comm_rank(const idocp_comm_t* c);
int idocp_comm_world(const idocp_comm_t* c);
int idocp_parnmpc_dist_attach(idocp_ocp_t* shard, idocp_comm_t* comm);
int idocp_parnmpc_dist_detach(idocp_ocp_t* shard);
/* rank 0: the measured state q[batch][nq], v[batch][nv] (host buffers) */
int idocp_parnmpc_dist_set_initial_state(idocp_ocp_t* shard, const double* q, const double* v, int nq, int nv);
int idocp_parnmpc_dist_init_backward_correction(idocp_ocp_t* shard, double t);
/* One iteration of the whole horizon; returns when everything is enqueued (idocp_ocp_synchronize before reading results). */
int idocp_parnmpc_dist_update_solution(idocp_ocp_t* shard, double t);
/* ... with the filter line search on the primal step (ParNMPCSolver::updateSolution(t, q, v, true)): collective like the call above;
 * host-synchronous (one device-to-host copy of the all-reduced sums per probe, like the single-handle path). */
int idocp_parnmpc_dist_update_solution_ls(idocp_ocp_t* shard, double t);
/* KKT error of the whole horizon on every rank, kkt_error[batch] (host). */
int idocp_parnmpc_dist_kkt_error(idocp_ocp_t* shard, double t, double* kkt_error);
int idocp_ocp_batch(idocp_ocp_t* h);
/* Storage precision of the Riccati factorisation P, s of OCPSolver: bits = 64 (default) or 32 (every entry of the cost-to-go rounded to
 * single precision when a stage of the backward sweep stores it; the arithmetic stays FP64).  BASELINE.json configs[4]'s tolerance study
 * on the device (tests/test_hybrid_gpu.py::test_configs4_grid_and_fp32_storage); FP64 is the product's precision. */
int idocp_ocp_set_riccati_storage(idocp_ocp_t* h, int bits);
/* dimensions of the configuration / velocity the handle's model has (q[batch][nq], v[batch][nv] of the update entries) */
int idocp_ocp_state_dims(idocp_ocp_t* h, int* nq, int* nv);
/* Test switches of the transport (tests/test_rccl_gpu.py; the one-GPU box cannot run more than one rank):
 *  idocp_comm_set_force_collectives   world == 1: issue all-reduce / broadcast through RCCL anyway instead of skipping them
 *  idocp_parnmpc_dist_transport_selftest   world 1: grouped ncclSend / ncclRecv of every halo kind to this very rank, all-reduce (sum, min)
 *                                          and broadcast on the shard's stream.  world > 1 (COLLECTIVE: every rank calls it; bench.py does
 *                                          before the timed region): every halo kind to the right neighbour and from the left one in one
 *                                          group, then the other way round -- the grouping of the driver's boundary exchange
 *                                          (backward_correction_solver.cpp:255-366 is what those halos feed) --, a pattern that names kind,
 *                                          element and sending rank; all-reduce (sum, min) and broadcast against their closed forms.
 *                                          *max_abs_diff = deviation of what came back (0 expected)
 *  idocp_comm_info                         what the communicator reports about itself: ncclCommCount, ncclCommUserRank, ncclGetVersion
 *                                          (any pointer may be NULL; transport: 1 RCCL, 0 the in-process test transport) */
int idocp_comm_set_force_collectives(idocp_comm_t* c, int on);
int idocp_parnmpc_dist_transport_selftest(idocp_ocp_t* shard, double* max_abs_diff);
int idocp_comm_info(const idocp_comm_t* c, int* nranks, int* user_rank, int* rccl_version, int* transport);
/* Deep copy of a solver handle (the reference's solver classes are copyable): same configuration, device records, contact
 * sequence and discretisation. */
int idocp_ocp_clone(idocp_ocp_t* src, idocp_ocp_t** out);
/* Replace the cost of a solver (OCPSolver / ParNMPCSolver handles).  The reference's solvers share the
 * CostFunction with the driver (ocp_solver.hpp:37-39: shared_ptr), so references and weights changed
 * between two updateSolution calls take effect at the next one; here the cost is copied at creation and
 * this call is how an MPC loop moves its goal.  A task-space cost cannot be added or removed
 * (IDOCP_E_UNSUPPORTED).  Takes effect with the next call that discretises the horizon. */
int idocp_ocp_set_cost(idocp_ocp_t* h, const idocp_cost_t* cost);
/* Device pointers of the state in front of the first stage (q[batch][nq], v[batch][nv]) and of
 * the step sizes ([batch][2]: primal, dual) -- the latter is all-reduced (min) between phases 8 and 9. */
int idocp_parnmpc_prev_state(idocp_ocp_t* h, double** d_q, double** d_v);
int idocp_parnmpc_step_sizes_device(idocp_ocp_t* h, double** d_steps);
/* Filter line search of ParNMPCSolver on a sharded horizon (round 4; src/line_search/line_search.cpp:199-301 evaluates every stage against
 * the trial iterate of its predecessor -- across a cut that is the left neighbour's trial iterate -- and sums over the horizon): the pieces
 * the sharded driver puts together.  idocp_parnmpc_set_line_search_hooks installs the two collective steps of one probe (pre: after the
 * trial iterate is formed; post: after the shard's cost / violation sums are formed); idocp_parnmpc_trial_halo_async packs / unpacks the
 * state_last halo of the trial iterate; idocp_parnmpc_merit_device gives the sums [batch][2] to all-reduce; idocp_parnmpc_line_search runs
 * LineSearch::computeStepSize on the direction of phases 0 .. 8 (every shard calls it: the filters evolve identically on identical sums).
 * Application code calls idocp_parnmpc_dist_update_solution_ls. */
int idocp_parnmpc_set_line_search_hooks(idocp_ocp_t* h, int (*pre)(idocp_ocp_t*), int (*post)(idocp_ocp_t*));
int idocp_parnmpc_trial_halo_async(idocp_ocp_t* h, int do_import, double* d_buf);
int idocp_parnmpc_merit_device(idocp_ocp_t* h, double** d_merit);
int idocp_parnmpc_line_search(idocp_ocp_t* h);
/* Discretise at time t (stage references, constraint levels) before launching phases by hand. */
int idocp_parnmpc_discretize(idocp_ocp_t* h, double t);
/* Squared KKT error of this shard's stages, d_err2[batch] in device memory (summed over the ranks by
 * the caller); the state in front of the first stage is the one held on the device. */
int idocp_parnmpc_kkt_error_squared_device(idocp_ocp_t* h, double t, double* d_err2);
/* Device-to-device copy (moving halos between the library's buffers and the caller's). */
int idocp_device_copy(void* d_dst, const void* d_src, unsigned long nbytes);

/* One kernel launch: 0 = tangent RNEA, 1 = condense, 2 = backward Riccati,
 * 3 = forward Riccati, 4 = expand primal, 5 = step-size reduction,
 * 6 = expand dual + integrate; 7 and 8 = the two halves of 1 (7: the nominal
 * rigid-body sweeps and the rows of the external terms, 8: the condensation
 * launches), so that a profiler of the caller can bracket them apart.
 * Since round 5 the forward sweep of a BATCH of instances expands as it walks (riccati_recursion_solver.cpp:129-251 in one kernel): id 3
 * is then the whole of 3 + 4 + 5 and ids 4, 5 launch nothing; idocp_ocp_fused_forward(h) says which form the handle runs (small batches
 * keep the three kernels: latency mode, below batch 192; idocp_ocp_set_fused_forward forces one form). */
int idocp_ocp_launch_kernel(idocp_ocp_t* h, int kernel_id, const double* d_q,
                            const double* d_v);
int idocp_ocp_fused_forward(idocp_ocp_t* h);
/* mode -1: by batch size (default); 0: S4 + K6 + reduction; 1: the fused forward sweep -- per handle (tuning / the parity tests of both forms) */
int idocp_ocp_set_fused_forward(idocp_ocp_t* h, int mode);

/* The backward Riccati sweep S3 (riccati_recursion_solver.cpp:48-107) has two forms: one wavefront per instance with P in registers (batches:
 * the throughput form) and eight wavefronts per instance with P staged in LDS (a handful of instances: the latency form, 8 % faster at batch
 * 1).  idocp_ocp_riccati_sweep(h): 1 when the handle runs the latency form.  set: mode -1 by batch size (default: batch <= 16 ->
 * latency form), 0 throughput form, 1 latency form -- per handle, copied by clone. */
int idocp_ocp_riccati_sweep(idocp_ocp_t* h);
int idocp_ocp_set_riccati_sweep(idocp_ocp_t* h, int mode);

/* Fork / join inside an iteration of an OCPSolver handle: the switching-constraint kernel K5s (next to the nominal sweeps) and the base poses
 * K7b (next to K7) run on a stream of the handle's own; every entry point joins before it reads or launches.  idocp_ocp_side_stream(h): 1
 * when the handle has that stream.  set: mode -1 by batch size (default: from batch 128), 0 everything on the handle's stream, 1 the side
 * stream -- per handle, copied by clone; the call waits for the handle's work, then creates or destroys the stream.  The answers are bitwise
 * the same in both forms. */
int idocp_ocp_side_stream(idocp_ocp_t* h);
int idocp_ocp_set_side_stream(idocp_ocp_t* h, int mode);

/* ---- Batched rigid-body terms on plain arrays: what Robot::RNEA, RNEADerivatives, setContactForces,
 * computeBaumgarteResidual / Derivatives, RNEAImpulse(+Derivatives), computeImpulseVelocityResidual / Derivatives and computeMJtJinv
 * (include/idocp/robot/robot.hxx:85-91, 262-283, 444-540, 576-615; contact_dynamics.hxx:105-158) give the reference, for n independent
 * samples in one launch.  The handle uploads the model once and owns a stream; calls are ordered on it.
 * Accepted models: a floating-base quadruped (4 legs x 3 revolute joints, 4 point contacts on the tip joints; every output), or a
 * fixed-base serial chain of 2 .. 8 revolute joints (tau and dtau_* only: f, contact_points and the contact outputs must be NULL).
 * Anything else returns IDOCP_E_UNSUPPORTED and idocp_last_error() names these shapes.  Without a GPU: IDOCP_E_DEVICE, no CPU fallback. */
typedef struct idocp_rbd idocp_rbd_t;
int idocp_rbd_create(const idocp_model_t* model, int device, idocp_rbd_t** out);
void idocp_rbd_destroy(idocp_rbd_t* h);
int idocp_rbd_synchronize(idocp_rbd_t* h);
void* idocp_rbd_stream(idocp_rbd_t* h);      /* hipStream_t */

#define IDOCP_RBD_STAGE 0    /* ID with gravity, Baumgarte constraint */
#define IDOCP_RBD_IMPULSE 1  /* RNEAImpulse: no gravity, v = 0 in the dynamics, a = dv; impulse velocity constraint at v + dv */

/* n samples; every pointer is host memory (idocp_rbd_contact_dynamics_batch) or device memory (..._batch_device).  Outputs that are NULL
 * are neither computed nor stored.  Matrices are column-major.  Rows of an inactive contact in C and dC* are zero, its f is ignored. */
typedef struct idocp_rbd_io {
  const double *q, *v, *a;      /* [n][nq], [n][nv], [n][nv] */
  const double *f;              /* [n][ncontacts][3], local contact-frame coordinates; NULL = 0 */
  const double *contact_points; /* [n][ncontacts][3]; needed for C in STAGE mode */
  double *tau, *dtau_dq, *dtau_dv, *dtau_da; /* [n][nv], [n][nv * nv] */
  double *C, *dCdq, *dCdv, *dCda;            /* [n][3 ncontacts], [n][3 ncontacts * nv]; IMPULSE: dCdv and dCda both hold d C / d (v + dv) */
  double *MJtJinv;              /* [n][(nv + 3 ncontacts)^2] slot; the inverse of [M J^T; J 0] over the active rows (J = dCda), packed
                                 * (nv + dimf)^2 column-major at the start of the slot like idocp_ocp_get_contact_dynamics packs it;
                                 * NaN where M or J M^-1 J^T is not positive definite.  The rest of a slot behind the packed block
                                 * (dimf < 3 ncontacts): zero in the host form, UNSPECIFIED in the device form (left as it was) */
} idocp_rbd_io_t;

/* active[ncontacts]: contact status shared by the n samples (NULL on a chain); time_step: the Baumgarte time step (STAGE mode with a
 * contact output).  The host form returns when the outputs are in place; it stages through buffers the handle owns and grows. */
int idocp_rbd_contact_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io);
/* Asynchronous on idocp_rbd_stream(h); allocates nothing on a quadruped, and on a chain only when n grows. */
int idocp_rbd_contact_dynamics_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io);

/* ---- Forward dynamics with contacts, the explicit Euler step and a rollout (an ADDITION: the reference has no counterpart; it only ever
 * evaluates the inverse direction).  Defined through the call above:
 *   STAGE    (a, f) is the pair for which idocp_rbd_contact_dynamics_batch(STAGE, q, v, a, f) returns tau = S^T u ([0_6; u] on a quadruped, u
 *            on a chain) and C = 0 on the active rows:  [M J^T; J 0] [a; -f] = [S^T u - h; -b],  h = ID(q, v, 0, 0), b = C(q, v, 0).
 *   IMPULSE  (dv, lambda) is the pair for which the IMPULSE call returns tau = 0 and a zero impulse-velocity constraint at v + dv on the
 *            active rows:  [M J^T; J 0] [dv; -lambda] = [0; -J v].  u is ignored.
 * A fixed-base chain has STAGE mode only, a = M^-1 (u - h); f and contact_points must be NULL.  The 42 x 42 inverse is never formed: M^-1 by
 * the block-arrow inverse, one Cholesky solve of J M^-1 J^T over the active rows.  Where M or J M^-1 J^T is not positive definite every
 * output of that sample is NaN (the convention of MJtJinv).
 * Outputs left NULL are neither computed nor stored.  q_next may be the very pointer q and v_next the very pointer v (a sample's q and v are
 * read completely before anything of that sample is written); no other overlap of inputs and outputs is allowed. */
typedef struct idocp_rbd_fd_io {
  const double *q, *v;           /* [n][nq], [n][nv] */
  const double *u;               /* [n][nu] joint torques; NULL = 0; ignored in IMPULSE mode */
  const double *contact_points;  /* [n][ncontacts][3]; needed in STAGE mode with an active contact */
  double *a;                     /* [n][nv]: STAGE the acceleration, IMPULSE the velocity jump dv */
  double *f;                     /* [n][ncontacts][3], local contact-frame coordinates, zero where inactive; IMPULSE: the impulse lambda */
  double *q_next, *v_next;       /* [n][nq], [n][nv]: the explicit Euler step of the OCP's own discretisation over dt (state_equation.hxx):
                                  * STAGE q (+) dt v (the SE(3) retraction of idocp_model_integrate_configuration on a floating base, the
                                  * quaternion normalised like there), v + dt a; IMPULSE q, v + dv */
} idocp_rbd_fd_io_t;
/* active[ncontacts]: contact (STAGE) or impulse (IMPULSE) status shared by the n samples, NULL on a chain; time_step: the Baumgarte time step
 * (positive in STAGE mode with an active contact); dt: the integration step (finite; only q_next / v_next see it). */
int idocp_rbd_forward_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing on a quadruped, and on a chain only when n grows. */
int idocp_rbd_forward_dynamics_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt,
                                            const idocp_rbd_fd_io_t* io);

/* `steps` forward-dynamics launches with the Euler step, chained on the handle's stream without a synchronisation in between.  Step-major
 * arrays, so that every step reads and writes one contiguous slice:
 *   q_traj [steps + 1][n][nq], v_traj [steps + 1][n][nv] (slice 0 is the input), u [steps][n][nu] (NULL = 0), optional a_traj [steps][n][nv],
 *   f_traj [steps][n][ncontacts][3]; active [steps][ncontacts] (shared by the n samples; NULL on a chain), contact_points
 *   [steps][n][ncontacts][3] (NULL on a chain).
 * touchdown_impulse != 0: a step k >= 1 whose status activates contacts that the status of step k - 1 did not have is preceded by one IMPULSE
 * solve whose impulse status is exactly the newly active contacts (what DiscreteEvent::setDiscreteEvent makes of the two statuses).  The
 * stored slice k of v_traj is then the POST-impulse velocity, i.e. the velocity the Euler step k is applied from (slice k was the
 * pre-impulse velocity until then; it is overwritten in place), and v_traj[k + 1] = v_traj[k] + dt a_traj[k] holds for every k.  The impulse
 * itself is not returned.  Step 0 never takes an impulse.
 * The host form stages everything once and reads back once; the device form allocates nothing on a quadruped. */
int idocp_rbd_rollout(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u,
                      const double* contact_points, double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse);
int idocp_rbd_rollout_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u,
                             const double* contact_points, double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse);

/* ---- Derivatives of the forward dynamics and the linearised Euler step (an ADDITION like the forward dynamics; rbd_fd_derivatives_kernel.hip).
 * At the forward solution (a, f) of [M J^T; J 0] [a; -f] = [S^T u - h; -b], with theta = q (in the tangent q (+) eps e_r of
 * idocp_model_integrate_configuration) or v, differentiating ID(q, v, a, f) = S^T u and C(q, v, a) = 0 gives
 *   d[a; -f]/dtheta = -MJtJinv [dID/dtheta ; dC/dtheta],      d[a; -f]/du = MJtJinv[:, 0 : nv] S^T,
 * every block the one idocp_rbd_contact_dynamics_batch returns at (q, v, a, f), over the active rows.  The call is that composition: the forward
 * launch, the inverse launch at its solution into scratch the handle owns, and one kernel that forms the products.  The scratch only grows
 * and is CAPPED at 256 MiB whatever n is: a larger call takes the sample axis in several passes on the handle's stream.
 * Inputs are those of idocp_rbd_fd_io_t.  Every output is optional and column-major; a NULL output is not stored (the products are formed
 * all the same, so that a sample's bits do not depend on what was asked for):
 *   a, f                 as idocp_rbd_forward_dynamics_batch returns them, bit for bit
 *   da_dq, da_dv         [n][nv * nv]            da_du  [n][nv * nu]
 *   df_dq, df_dv         [n][3 ncontacts * nv]   df_du  [n][3 ncontacts * nu]; the rows of inactive contacts are zero; the sign is that of f
 *   A [n][2 nv * 2 nv], B [n][2 nv * nu]: the Jacobians of the OCP's explicit Euler step x_next = (q (+) dt v, v + dt a) with respect to
 *     x = [dq; dv] and u.  Column r of the top rows of A is d/d eps [(q (+) eps e_r (+) dt v) (-) (q (+) dt v)] at eps = 0 -- it lives in the
 *     tangent at q_next; (+) / (-) are idocp_model_integrate_configuration / idocp_model_subtract_configuration.  The bottom rows of A are
 *     [dt da_dq, I + dt da_dv]; B = [0; dt da_du].  On a chain the top rows of A are [I, dt I].
 * IMPULSE mode: a is dv and f is lambda; u and the *_du outputs must be NULL; A is the Jacobian of (q, v + dv), top rows [I 0]; B must be NULL.
 * A fixed-base chain takes STAGE mode only (da_dq = -M^-1 dtau/dq, da_dv = -M^-1 dtau/dv, da_du = M^-1), and its contact outputs must be NULL.
 * Where M or J M^-1 J^T of a sample is not positive definite, or an input of that sample is not finite, every output of that sample is NaN and
 * no other sample is touched.  A sample's bits depend neither on n, nor on the outputs that were asked for, nor on how the sample axis was cut.
 * No input may overlap an output.  IDOCP_E_ARG with a text in idocp_last_error() for everything refused. */
typedef struct idocp_rbd_fdd_io {
  const double *q, *v, *u, *contact_points;   /* as in idocp_rbd_fd_io_t */
  double *a, *f;
  double *da_dq, *da_dv, *da_du;
  double *df_dq, *df_dv, *df_du;
  double *A, *B;
} idocp_rbd_fdd_io_t;
/* ADDITION.  Host pointers; stages through the handle's buffers and returns when the outputs are in place. */
int idocp_rbd_forward_dynamics_derivatives_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt,
                                                 const idocp_rbd_fdd_io_t* io);
/* ADDITION.  Device pointers; asynchronous on idocp_rbd_stream(h); allocates only when the scratch has to grow. */
int idocp_rbd_forward_dynamics_derivatives_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt,
                                                        const idocp_rbd_fdd_io_t* io);
/* ADDITION.  Linearises a trajectory that idocp_rbd_rollout / _policy / _footholds has ALREADY produced, about the torques that were applied:
 *   u_traj [steps][n][nu] (NULL = 0), contact_points [steps][n][ncontacts][3], q_traj [steps + 1][n][nq], v_traj [steps + 1][n][nv]: inputs;
 *   A_traj [steps][n][2 nv * 2 nv], B_traj [steps][n][2 nv * nu]: outputs, step-major, column-major blocks; either may be NULL.
 * A_traj[k] is the Jacobian of STORED slice k + 1 with respect to STORED slice k, so that the product of the A_traj[k] is the sensitivity of what
 * the rollout stored.  Where step k + 1 carries a touchdown impulse (the rule of idocp_rbd_rollout, touchdown_impulse != 0), stored slice k + 1 is
 * post-impulse: A_traj[k] = E A_k and B_traj[k] = E B_k, with A_k, B_k of the call above on slice k and E the IMPULSE-mode A of that call at
 * (q_traj[k + 1], v_traj[k] + dt a) -- the pre-impulse velocity is recomputed, not read from slice k + 1 -- with the newly active contacts.
 * Elsewhere E = I.  The contact points are held FIXED: the latch of idocp_rbd_rollout_footholds is not differentiated, nor is the clamp of a
 * policy.  Asynchronous on the handle's stream in the device form, without a synchronisation between the steps. */
int idocp_rbd_linearize_rollout(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u_traj,
                                const double* contact_points, const double* q_traj, const double* v_traj, double* A_traj, double* B_traj,
                                int touchdown_impulse);
int idocp_rbd_linearize_rollout_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u_traj,
                                       const double* contact_points, const double* q_traj, const double* v_traj, double* A_traj, double* B_traj,
                                       int touchdown_impulse);

/* ---- Closed loop: the time-varying affine feedback policy of the solvers on the plant above (an ADDITION like the forward dynamics).  Before
 * every step
 *   u = clamp(u_ff[k] + K[k] [q (-) q_ref[k] ; v - v_ref[k]])
 * is evaluated on the GPU (rbd_policy_kernel.hip), without a host round trip.  K[k] is nu x 2 nv column-major with the columns [dq | dv]: the
 * block idocp_ocp_get_riccati returns, and [Kq | Kv] of getStateFeedbackGain / idocp_unocp_get_torque_feedback_gain.  q (-) q_ref is the tangent
 * idocp_model_subtract_configuration(q_plus = q, q_minus = q_ref) returns (SE(3) log of the relative base placement in rows 0 .. 5 on a
 * quadruped, plain differences elsewhere; quaternions are taken as given).  The clamp min(max(u, u_min), u_max) per joint is the last operation.
 * A non-finite entry in a sample's q, v, q_ref, v_ref, K or u_ff makes all of that sample's torques NaN and touches no other sample.
 * Gains and references are per sample, or one set shared by all n samples (one policy over many perturbed plants). */
typedef struct idocp_rbd_policy {
  const double *u_ff;          /* [steps][n][nu]; NULL = 0 */
  const double *K;             /* [steps][n][nu * 2 nv], or [steps][nu * 2 nv] if shared_gains; NULL = no feedback (q_ref, v_ref are not read) */
  const double *q_ref, *v_ref; /* [steps][n][nq | nv], or [steps][nq | nv] if shared_ref; required when K is given */
  const double *u_min, *u_max; /* [nu], either may be NULL (unbounded on that side) */
  int shared_gains, shared_ref;
} idocp_rbd_policy_t;

/* One evaluation (the steps = 1 slices of the policy): u [n][nu] from q [n][nq], v [n][nv].  Host pointers; returns when u is in place.
 * IDOCP_E_ARG for a null policy, K without q_ref or v_ref, and a bound pair with u_min[j] > u_max[j] or a NaN bound. */
int idocp_rbd_feedback_torques_batch(idocp_rbd_t* h, int n, const double* q, const double* v, const idocp_rbd_policy_t* policy, double* u);
/* Device pointers for everything, u_min and u_max included; asynchronous on idocp_rbd_stream(h); allocates nothing.  The bounds are NOT
 * checked (they are device memory). */
int idocp_rbd_feedback_torques_batch_device(idocp_rbd_t* h, int n, const double* q, const double* v, const idocp_rbd_policy_t* policy, double* u);

/* idocp_rbd_rollout with the torques of step k computed from the state of step k.  Array shapes, schedule and touchdown rules are those of
 * idocp_rbd_rollout; per step: the touchdown impulse if any, the policy launch, the forward launch, all on the handle's stream with no
 * synchronisation in between.  The policy of step k sees the state the Euler step k is applied from -- with a touchdown the POST-impulse
 * velocity, which is what slice k of v_traj holds afterwards.  u_traj [steps][n][nu] receives the torques applied; NULL: a buffer of n nu
 * doubles the handle owns (it grows only when n grows).  The host form stages everything once and reads back once and refuses bad bounds like
 * the call above; the device form takes device pointers for everything, does not check the bounds and allocates nothing beyond that buffer
 * (a chain also grows the buffers of idocp_rbd_rollout_device). */
int idocp_rbd_rollout_policy(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const idocp_rbd_policy_t* policy,
                             const double* contact_points, double* q_traj, double* v_traj, double* u_traj, double* a_traj, double* f_traj,
                             int touchdown_impulse);
int idocp_rbd_rollout_policy_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt,
                                    const idocp_rbd_policy_t* policy, const double* contact_points, double* q_traj, double* v_traj, double* u_traj,
                                    double* a_traj, double* f_traj, int touchdown_impulse);

/* ---- Time-varying LQR gains about a linearised rollout: the backward pass of LQR / iLQR per sample, on the GPU (rbd_lqr_kernel.hip; an ADDITION
 * like the rest of this block, the reference has no counterpart).  It consumes what idocp_rbd_linearize_rollout writes and produces gains in
 * exactly the layout idocp_rbd_policy_t reads, so that rollout, linearisation, gains, policy rollout and score run on the handle's stream with no
 * host round trip.  With W* = diag(*_weight), the recursion -- this is the definition -- is
 *   P = Wxf, p = lx[steps];   for k = steps - 1 .. 0, with A = A_traj[k], B = B_traj[k]:
 *     Qx = lx[k] + A^T p,  Qu = lu[k] + B^T p,
 *     Qxx = Wx + A^T P A,  Qux = B^T P A,  Quu = Wu + regularization I + B^T P B,
 *     K_k = -Quu^-1 Qux,  k_k = -Quu^-1 Qu   (Cholesky),
 *     P <- (X + X^T) / 2 with X = Qxx + Qux^T K_k,   p <- Qx + Qux^T k_k.
 * The sign is the policy's, u = u_ff + K e: a caller sets u_ff = u_traj (+ alpha k_traj), q_ref = q_traj, v_ref = v_traj with shared_ref = 0, and
 * K = K_traj, unchanged.  The weights are diagonal and already scaled by the caller (dt included); the a_weight and f_weight terms of
 * idocp_cost_t have no place in a diagonal x_weight / u_weight.  Both model kinds are taken (quadruped: 2 nv = 36, nu = 12; chains of 2 .. 8
 * joints).  An output that is NULL is not stored; a sample's bits depend neither on n, nor on the outputs asked for, nor on the form of the call.
 * Failure is per sample: a sample fails at step k if a pivot of Quu at step k is not positive or an entry the step reads from that sample is not
 * finite.  K_traj and k_traj of the steps <= k, P0, p0 and expected of that sample are then NaN and status = k; the steps > k keep their valid
 * values, and no other sample is touched. */
typedef struct idocp_rbd_lqr_io {
  const double *A_traj, *B_traj;   /* [steps][n][2nv*2nv], [steps][n][2nv*nu]: exactly what idocp_rbd_linearize_rollout writes */
  const double *x_weight;          /* [2nv] stage weight on [dq; dv], diagonal, >= 0, already scaled by the caller (dt included) */
  const double *u_weight;          /* [nu]  stage weight on du, >= 0 */
  const double *xf_weight;         /* [2nv] terminal weight, >= 0 */
  const double *lx_traj, *lu_traj; /* optional cost gradients [steps + 1][n][2nv], [steps][n][nu]; both or neither; NULL = 0 */
  double regularization;           /* >= 0, added to the diagonal of Quu */
  double *K_traj;                  /* [steps][n][nu * 2nv], column-major nu x 2nv, columns [dq | dv]: the K of idocp_rbd_policy_t */
  double *k_traj;                  /* [steps][n][nu] feed-forward step; only with gradients */
  double *P0, *p0;                 /* [n][2nv*2nv], [n][2nv]: value function at slice 0 */
  double *expected;                /* [n][2]: {sum_k k_k^T Qu_k, 1/2 sum_k k_k^T Quu_k k_k}; only with gradients */
  int *status;                     /* [n]: -1, or the largest step index at which the sample failed */
} idocp_rbd_lqr_io_t;
/* Host pointers; stages through the handle's buffer like the other host forms and returns when the outputs are in place.  IDOCP_E_ARG (the text
 * of idocp_last_error names the call) for n <= 0, steps < 1, a NULL handle, io, A_traj, B_traj or weight array, only one of lx_traj / lu_traj,
 * k_traj or expected without gradients, no output at all, a negative or non-finite regularization, and a negative or non-finite weight. */
int idocp_rbd_lqr_backward(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io);
/* Device pointers for everything, the weights and status included; asynchronous on idocp_rbd_stream(h); allocates nothing.  The weights are
 * NOT checked (they are device memory). */
int idocp_rbd_lqr_backward_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io);

/* ---- Contact-frame kinematics for n states (rbd_kinematics_kernel.hip): the batched counterpart of Robot::updateFrameKinematics with
 * getContactPoints, frameRotation and getFrameJacobian, which idocp_model_contact_positions / idocp_model_frame_world_placement give one state
 * on the host.  Quadrupeds only (a fixed-base chain has no contact frames: IDOCP_E_UNSUPPORTED).  Per sample i and contact c:
 *   points   [n][nc][3]      world position of the contact frame origin, the quantity idocp_model_contact_positions returns
 *   rotation [n][nc][9]      world rotation of the contact frame, row-major: it takes the local force coordinates of f_traj to the world frame
 *   velocity [n][nc][3]      world-frame linear velocity of the frame origin: d/d eps points(q (+) eps v) at eps = 0, (+) the retraction of
 *                            idocp_model_integrate_configuration; equal to rotation times the LOCAL linear frame velocity.  Needs v.
 *   jacobian [n][3 nc * nv]  the 3 nc x nv matrix J, column-major: column r is d/d eps points(q (+) eps e_r), so velocity = J v.  Every entry
 *                            is written, the structural zeros of the other legs' columns included.  This is the WORLD-frame Jacobian; dCda
 *                            of idocp_rbd_contact_dynamics_batch is the LOCAL one: its rows of contact c are rotation[c]^T times these.
 * A NULL output is neither computed nor stored.  The quaternion is taken as given.  A sample's results are bit for bit the same alone or in a
 * batch and for any selection of outputs.  A non-finite entry in a sample's q makes all of that sample's outputs NaN, one in its v the
 * sample's velocity, and touches no other sample. */
typedef struct idocp_rbd_kin_io {
  const double *q, *v;                       /* [n][nq], [n][nv]; v only for velocity */
  double *points, *rotation, *velocity, *jacobian;
} idocp_rbd_kin_io_t;
/* ADDITION.  Host pointers; returns when the outputs are in place.  IDOCP_E_ARG for n <= 0, a null handle, io or q, velocity without v and no
 * output at all. */
int idocp_rbd_contact_kinematics_batch(idocp_rbd_t* h, int n, const idocp_rbd_kin_io_t* io);
/* ADDITION.  Device pointers; asynchronous on idocp_rbd_stream(h); one launch; allocates nothing. */
int idocp_rbd_contact_kinematics_batch_device(idocp_rbd_t* h, int n, const idocp_rbd_kin_io_t* io);

/* ---- A rollout that latches its footholds: idocp_rbd_rollout / idocp_rbd_rollout_policy with contact_points an IN / OUT trajectory, so that a
 * schedule with lift-offs and touchdowns anchors every plant where ITS foot is.  With
 *   stays(k, c) = active[k][c] && (k > 0 ? active[k - 1][c] : !latch_first)
 * slice k of contact_points [steps][n][nc][3] is, per sample i and contact c,
 *   stays(k, c)   contact_points[k - 1][i][c], carried bit for bit (at k = 0: the caller's value, left as it is)
 *   otherwise     points_c(q_traj[k][i]) of the call above: the foot at the state the Euler step k is applied from (a touchdown impulse
 *                 changes v, not q).
 * A contact that becomes active is anchored at that plant's foot, and the entry of an open contact tracks the swing foot: every slice is fully
 * defined and doubles as the foot trajectory.  Only slice 0 is read, and of it only the contacts active at step 0 with latch_first == 0.
 * Everything else -- array shapes, the touchdown impulse on the newly active contacts, the policy before the forward launch, the NaN
 * conventions -- is idocp_rbd_rollout (u given), idocp_rbd_rollout_policy (policy given) or idocp_rbd_rollout with u = NULL (neither); u
 * together with policy is IDOCP_E_ARG.  Feeding the contact_points this call produced into those calls reproduces its trajectories bit for
 * bit.  Per step: the latch launch, the touchdown impulse if any, the policy launch if any, the forward launch, all on the handle's stream
 * with no synchronisation in between.  Quadrupeds only (IDOCP_E_UNSUPPORTED on a chain). */
typedef struct idocp_rbd_foothold_rollout {
  const double* u;                   /* open loop [steps][n][nu], or NULL */
  const idocp_rbd_policy_t* policy;  /* closed loop, or NULL; u and policy both given: IDOCP_E_ARG; both NULL: zero torques */
  double* contact_points;            /* [steps][n][nc][3], IN (slice 0) / OUT (every slice) */
  double *q_traj, *v_traj, *u_traj, *a_traj, *f_traj;   /* as idocp_rbd_rollout_policy (u_traj is written only with a policy) */
} idocp_rbd_foothold_rollout_t;
/* ADDITION.  Host pointers (those of the policy included); stages everything once -- slice 0 of contact_points goes up, every slice comes back
 * -- and refuses bad policy bounds like idocp_rbd_rollout_policy.  contact_points, q_traj, v_traj and active are needed; time_step must be
 * positive if any step has an active contact. */
int idocp_rbd_rollout_footholds(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt,
                                const idocp_rbd_foothold_rollout_t* io, int touchdown_impulse, int latch_first);
/* ADDITION.  Device pointers for everything the struct and the policy point to (io and *policy themselves are host memory); asynchronous on
 * idocp_rbd_stream(h); allocates nothing beyond what idocp_rbd_rollout_policy_device may (the torque buffer when u_traj is NULL). */
int idocp_rbd_rollout_footholds_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt,
                                       const idocp_rbd_foothold_rollout_t* io, int touchdown_impulse, int latch_first);

/* ---- Scoring a rollout: the solvers' cost and a constraint violation per sample, on the GPU (rbd_score_kernel.hip).
 * The objective holds what scoring needs: the weights of an idocp_cost_t, the switches and bounds of an idocp_constraints_t (the joint limits
 * themselves are the model's q_min, q_max, v_max, u_max) and the configuration-space reference of every step t_k = t0 + k dt, k = 0 .. steps,
 * by the rules the solvers use (constant, use_trotting_ref, use_time_varying_ref; a chain takes the constant one).  The stored velocity
 * reference of a step is the one the cost compares with: v_ref (v_ref[0] = step_length / t_period under use_trotting_ref), zero outside the
 * window of use_time_varying_ref.
 * The cost mirrors what idocp_ocp_line_search_eval sums for a grid stage and the terminal stage of an iterate (SplitOCP::stageCost,
 * TerminalOCP::terminalCost), the barrier term left out; with e = q (-) q_ref(t_k), the tangent of idocp_model_subtract_configuration(q_plus = q,
 * q_minus = q_ref):
 *   stage_cost[k][i] = dt 1/2 (sum_r q_weight[r] e[r]^2 + v_weight[r] (v[r] - v_ref_k[r])^2 + a_weight[r] a[r]^2 + sum_j u_weight[j] (u[j] - u_ref[j])^2
 *                             + sum_{c active at step k} sum_x f_weight[c][x] (f[c][x] - f_ref[c][x])^2)
 *   terminal[i]      = 1/2 sum_r qf_weight[r] e[r]^2 + vf_weight[r] (v[r] - v_ref[r])^2      on the slice behind the last step
 *   cost[i]          = sum_k stage_cost[k][i] (+ terminal[i])
 * The violation is an ADDITION (the reference's |g + slack|_1 belongs to an interior-point iterate; a rollout has no slacks):
 *   violation[i] = sum_k dt sum_rows max(0, g_row)
 * over the rows switched on: per actuated joint q_min - q, q - q_max, -v_max - v, v - v_max, -u_max - u, u - u_max, a_min - a, a - a_max; per
 * contact active at step k the five rows of LinearizedFrictionCone (Jc f, Jc = {{0,0,-1},{1,0,-m},{-1,0,-m},{0,1,-m},{0,-1,-m}}, m = mu / sqrt 2)
 * or the two of FrictionCone (-fz, fx^2 + fy^2 - mu^2 fz^2).  The terminal slice has no constraints.
 * Not carried, refused by create with IDOCP_E_UNSUPPORTED: task-space cost components (task_dim != 0), contact_distance, both cones together,
 * and the trotting / time-varying reference on a chain.  The impulse-stage weights (qi_, vi_, dvi_, fi_weight) and the impulse cones are
 * ignored: a rollout does not return its touchdown impulses, so there is nothing to score them on.  barrier and fraction_to_boundary_rate are
 * not read. */
#define IDOCP_RBD_SCORE_MAX_WINDOW 1024      /* most steps of one scoring call */
typedef struct idocp_rbd_objective idocp_rbd_objective_t;
/* ADDITION.  constraints NULL: no rows.  dt positive, steps >= 1.  Uploads once, on the handle's stream, and returns when the upload is done;
 * nothing is allocated afterwards.  The objective belongs to the handle h and is destroyed before it. */
int idocp_rbd_objective_create(idocp_rbd_t* h, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double t0, double dt, int steps,
                               idocp_rbd_objective_t** out);
void idocp_rbd_objective_destroy(idocp_rbd_objective_t* o);
/* The reference of step k = 0 .. steps, host copy: q_ref [nq], v_ref [nv] (either may be NULL).  Mirrors the q_ref(t) the cost components
 * of the solvers form per stage (TrottingConfigurationSpaceCost::update_q_ref, TimeVaryingConfigurationSpaceCost::set_q_ref). */
int idocp_rbd_objective_get_reference(const idocp_rbd_objective_t* o, int k, double* q_ref, double* v_ref);
/* ADDITION.  The device tables [steps + 1][nq] and [steps + 1][nv], bit for bit what get_reference returns: directly usable as q_ref / v_ref of
 * an idocp_rbd_policy_t with shared_ref = 1 in the device form of the policy rollout.  They live as long as the objective. */
int idocp_rbd_objective_reference_device(const idocp_rbd_objective_t* o, const double** d_q_ref, const double** d_v_ref);

/* The step-major layout of idocp_rbd_rollout, so that its outputs can be passed straight in. */
typedef struct idocp_rbd_score_io {
  const double *q_traj, *v_traj;          /* [steps + 1][n][nq | nv] when terminal, else [steps][n][..]: the window's own slices */
  const double *u_traj, *a_traj, *f_traj; /* [steps][n][nu | nv | ncontacts * 3]; NULL is allowed only where no enabled weight or row reads the array
                                           * (else IDOCP_E_ARG naming it).  The f of a contact that is not active at a step is not read */
  double *cost, *violation;               /* [n]; either may be NULL */
  double *stage_cost;                     /* [steps (+ 1 when terminal)][n], the last slice the terminal cost; NULL = not stored */
} idocp_rbd_score_io_t;
/* ADDITION.  Scores the window of `steps` steps whose slice 0 is step first_step of the objective (first_step + steps <= the objective's steps; at
 * most IDOCP_RBD_SCORE_MAX_WINDOW steps per call).  active [steps][ncontacts]: the contact status per step, shared by the n samples (NULL on a
 * chain).  terminal != 0: the slice behind the last step of the window is scored with the terminal weights against the reference of step
 * first_step + steps.  accumulate != 0: adds to what cost / violation hold, so that a caller who keeps only a ring of slices scores window by
 * window.  One launch.  The sums are folded in a fixed order -- the rows of a step by a fixed tree, the steps in index order, the terminal
 * term last -- so a sample's results are bit for bit the same whatever n is, and whether it was scored at once or window by window.
 * A non-finite entry anywhere in the slices read of a sample (q, v, and u, a, f where given; an inactive contact's f is not read) makes both
 * of that sample's results NaN and touches no other sample; its stage_cost is unspecified.
 * Host pointers; returns when the results are in place. */
int idocp_rbd_score_rollout(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int terminal,
                            int accumulate, const idocp_rbd_score_io_t* io);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_score_rollout_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int terminal,
                                   int accumulate, const idocp_rbd_score_io_t* io);

/* ---- Gradients of an objective along a rollout (rbd_gradient_kernel.hip): the lx_traj, lu_traj that idocp_rbd_lqr_io_t reads.  An ADDITION.
 * This is the definition: the derivative of what idocp_rbd_score_rollout sums as `cost`, taken in the tangent x = [dq; dv], q (+) eps e_r, the tangent
 * of idocp_rbd_linearize_rollout.  With e = q (-) q_ref(t_k) and J = d e / d dq -- on the quadruped the base rows of J are the 6 x 6 Jlog6 of the
 * relative base placement and J is the identity elsewhere, on a chain J is the identity --, slice k of the window:
 *   lx[k][i][0:nv]   = dt J^T (q_weight o e)
 *   lx[k][i][nv:2nv] = dt v_weight o (v - v_ref_k)
 *   lu[k][i]         = dt u_weight o (u - u_ref)        (0 where u_traj is NULL)
 * and the terminal slice the same with qf_weight, vf_weight and no dt.  The reference forms the same product in ConfigurationSpaceCost
 * (configuration_space_cost.cpp:292-328: lq += dt J^T W diff with Robot::dSubtractdConfigurationPlus on a floating base).  The logarithm is the one
 * the score takes (lieRelative, lieLog6 of dev_lie.hpp); J^T (W e) of the base rows is summed over the rows in index order.
 * The gradient is of `cost`, NOT of `violation`: the constraint rows of the objective are not differentiated.  Refused with IDOCP_E_UNSUPPORTED, never
 * dropped: an objective with a non-zero a_weight entry or a non-zero f_weight entry of any contact -- their gradients need da/dx and df/dx, and their
 * Hessians are dense, which the diagonal x_weight / u_weight of idocp_rbd_lqr_backward cannot hold.
 * n, first_step, steps and terminal mean what they mean for idocp_rbd_score_rollout; IDOCP_RBD_SCORE_MAX_WINDOW does not apply (the slices are
 * independent), only (steps + 1) * n must fit an int.  A non-finite entry in what a slice reads of a sample (q, v, and u where given) makes that
 * sample's lx and lu of that slice NaN and touches nothing else.  A sample's bits depend neither on n, nor on the outputs asked for, nor on the form
 * of the call. */
typedef struct idocp_rbd_gradient_io {
  const double *q_traj, *v_traj;   /* [steps (+ 1 if terminal)][n][nq | nv] */
  const double *u_traj;            /* [steps][n][nu]; NULL is allowed only when every u_weight is zero */
  double *lx_traj;                 /* [steps (+ 1 if terminal)][n][2nv]; either output may be NULL */
  double *lu_traj;                 /* [steps][n][nu] */
} idocp_rbd_gradient_io_t;
/* ADDITION.  Host pointers; stages through the handle's buffer and returns when the outputs are in place.  IDOCP_E_ARG (idocp_last_error names the
 * call) for a NULL handle, objective or io, an objective of another handle, n <= 0, steps < 1, a window outside the objective, q_traj or v_traj
 * missing, u_traj missing under a non-zero u_weight, and no output at all. */
int idocp_rbd_objective_gradients(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, int terminal,
                                  const idocp_rbd_gradient_io_t* io);
/* ADDITION.  Device pointers; asynchronous on idocp_rbd_stream(h); one launch; allocates nothing. */
int idocp_rbd_objective_gradients_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, int terminal,
                                         const idocp_rbd_gradient_io_t* io);
/* ADDITION.  The LQR weights of an objective as device tables that live as long as the objective (uploaded by idocp_rbd_objective_create), directly
 * usable in idocp_rbd_lqr_io_t: x_weight [2nv] = dt [q_weight; v_weight], u_weight [nu] = dt u_weight, xf_weight [2nv] = [qf_weight; vf_weight].
 * They are the diagonal Gauss-Newton approximation with J ~ I on the base rows: they approximate the HESSIAN only.  The gradients above are exact, so
 * the fixed point of an iteration built on both is not moved.  Any of the three places may be NULL.  Refuses what the gradient call refuses. */
int idocp_rbd_objective_lqr_weights_device(const idocp_rbd_objective_t* o, const double** d_x_weight, const double** d_u_weight,
                                           const double** d_xf_weight);
/* ADDITION.  The host twin: the same bits into x_weight [2nv], u_weight [nu], xf_weight [2nv] (any may be NULL). */
int idocp_rbd_objective_get_lqr_weights(const idocp_rbd_objective_t* o, double* x_weight, double* u_weight, double* xf_weight);

/* ---- The line-search step of iLQR (rbd_ilqr_kernel.hip).  ADDITIONS.
 * idocp_rbd_ilqr_step_torques: u_ff[k][i][:] = u_traj[k][i][:] + alpha[i] * k_traj[k][i][:] (the product rounded, then the sum), all [steps][n][nu],
 * alpha [n]; a sample whose alpha is 0 gets u_traj bit for bit, whatever k_traj holds.  One launch.  IDOCP_E_ARG for a NULL handle or array,
 * n <= 0, steps < 1. */
int idocp_rbd_ilqr_step_torques(idocp_rbd_t* h, int n, int steps, const double* u_traj, const double* k_traj, const double* alpha, double* u_ff);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_ilqr_step_torques_device(idocp_rbd_t* h, int n, int steps, const double* u_traj, const double* k_traj, const double* alpha,
                                       double* u_ff);
/* idocp_rbd_ilqr_accept: per sample, with merit = cost + penalty * violation (the combination of idocp_rbd_importance_weights), the trial is
 * ACCEPTED if and only if done[i] == 0, trial_cost[i] and trial_violation[i] are finite, and
 *   merit_trial <= merit + armijo * (alpha e0 + alpha^2 e1),   {e0, e1} = expected[i] of idocp_rbd_lqr_backward, alpha = alpha[i].
 * (A NaN in expected or alpha rejects.)  An accepted sample copies its slices of the trial arrays over the current ones -- q, v
 * [steps + 1][n][..], u [steps][n][nu], and a, f [steps][n][..] where both the current and the trial array are given --, overwrites cost[i] and
 * violation[i], sets done[i] = 1 and writes alpha_accepted[i] = alpha[i].  A rejected sample does only this: alpha[i] *= shrink, and where
 * alpha[i] < alpha_min afterwards, alpha[i] = 0; nothing else of it is touched.  A sample with done[i] != 0 is left alone entirely.  The copies are
 * selects on whole slices, no arithmetic on the data.  One launch. */
typedef struct idocp_rbd_ilqr_accept_io {
  double *q_traj, *v_traj, *u_traj, *a_traj, *f_traj;   /* the current trajectory, in / out; a_traj, f_traj optional */
  double *cost, *violation;                             /* [n] its scores, in / out */
  const double *trial_q, *trial_v, *trial_u, *trial_a, *trial_f;
  const double *trial_cost, *trial_violation;           /* [n] */
  const double *expected;                               /* [n][2] */
  double *alpha;                                        /* [n], in / out */
  int *done;                                            /* [n], in / out */
  double *alpha_accepted;                               /* [n]; written for the samples accepted by this call only */
  double penalty, armijo, shrink, alpha_min;
} idocp_rbd_ilqr_accept_io_t;
/* Host pointers; returns when everything is in place.  IDOCP_E_ARG for a NULL handle, io or needed array, n <= 0, steps < 1, and a penalty, armijo,
 * shrink or alpha_min that is negative or not finite. */
int idocp_rbd_ilqr_accept(idocp_rbd_t* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t* io);
/* Device pointers, done included; asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_ilqr_accept_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t* io);

/* ---- One iLQR iteration on the handle's stream.  ADDITION.  Chains, with no synchronisation and no host read in between:
 *   idocp_rbd_linearize_rollout_device about (q_traj, v_traj, u_traj); idocp_rbd_objective_gradients_device (first_step 0, terminal);
 *   idocp_rbd_lqr_backward_device with the objective's weights and `regularization`; then alpha = 1, done = 0, alpha_accepted = 0 and `trials`
 *   rounds of: step torques; idocp_rbd_rollout_policy_device into the trial arrays with u_ff = u + alpha k, K = K_traj, q_ref = q_traj,
 *   v_ref = v_traj, shared_ref = 0 and the caller's u_min, u_max; idocp_rbd_score_rollout_device with terminal = 1 (window by window with accumulate
 *   beyond IDOCP_RBD_SCORE_MAX_WINDOW steps); accept.
 * A sample accepted in an early round is simply rolled out again in the later rounds and that trial is ignored (done[i] != 0): simpler than
 * compaction, and the stream stays free of host decisions.  A sample whose LQR status is not -1 has a NaN k_traj, hence a NaN trial: it is never
 * accepted and keeps its trajectory, so failure stays per sample.  Quadrupeds roll out under the caller's FIXED contact_points (latching footholds is
 * out of scope); chains pass active = contact_points = NULL.  The objective needs at least `steps` steps; step k of the rollout is its step k.
 * The workspace is carved, in this order and each piece at an even number of doubles, into A_traj, B_traj, lx, lu, K_traj, k_traj, u_ff, the trial
 * q, v, u, a, f, the trial cost and violation, alpha [n] and done [n ints]. */
typedef struct idocp_rbd_ilqr_io {
  double *q_traj, *v_traj, *u_traj;   /* [steps + 1][n][nq | nv], [steps][n][nu]: the current rollout, in / out */
  double *a_traj, *f_traj;            /* [steps][n][nv | 3 ncontacts], in / out, optional (f_traj NULL on a chain) */
  double *cost, *violation;           /* [n]: its score under the objective with terminal = 1, in / out (the caller scores the first rollout once) */
  const double *u_min, *u_max;        /* [nu], either may be NULL */
  double regularization, armijo, shrink, alpha_min, penalty;
  int trials;                         /* >= 1 */
  double *alpha_accepted;             /* [n]: the step taken, 0 = none */
  int *lqr_status;                    /* [n]: status of idocp_rbd_lqr_backward */
  double *expected;                   /* [n][2]: expected of idocp_rbd_lqr_backward */
  void *workspace;                    /* DEVICE memory of idocp_rbd_ilqr_workspace_bytes(h, n, steps) bytes, 16-byte aligned; the host form ignores it */
} idocp_rbd_ilqr_io_t;
/* bytes of the workspace, 0 for a NULL handle, n <= 0 or steps < 1 */
unsigned long long idocp_rbd_ilqr_workspace_bytes(const idocp_rbd_t* h, int n, int steps);
/* Device pointers (the workspace included); asynchronous on idocp_rbd_stream(h); allocates nothing beyond what the calls it chains may allocate. */
int idocp_rbd_ilqr_iterate_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                  const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);
/* Host pointers; stages once, owns its workspace for the duration of the call (in the handle's staging buffer) and reads back once. */
int idocp_rbd_ilqr_iterate(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                           const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);

/* ---- iLQR on the full cost: the acceleration and contact-force terms as Gauss-Newton residual rows (rbd_residual_kernel.hip, the GN form of
 * rbd_lqr_kernel.hip).  ADDITIONS.  The calls above refuse an objective with a non-zero a_weight or f_weight and keep doing so; the calls below
 * take every objective the score takes.  With nx = 2 nv, nz = nx + nu and R = roundup4(nv + 3 ncontacts) (32 on the quadruped, 4 or 8 on a chain),
 * the extra cost of stage k is 1/2 |rho|^2 and G = d rho / d [dq; dv; du] -- this is the definition:
 *   rows r < nv:        rho_r = s_r a_r,                       G[r][:] = s_r [da_r/dq | da_r/dv | da_r/du],  s_r = sqrt(dt a_weight[r])
 *   rows nv + 3 c + x:  rho = s (f[c][x] - f_ref[c][x]),       G       = s [df/dq | df/dv | df/du],          s = sqrt(dt f_weight[c][x])
 *                       where contact c is active at step k, else rho and the row of G are zero
 *   the rows behind nv + 3 ncontacts (padding) are zero.
 * a, f and the derivative blocks are those idocp_rbd_forward_dynamics_derivatives_batch returns in STAGE mode at slice k (also where step k + 1
 * carries a touchdown impulse: impulses are not scored).  s is the correctly rounded square root of the rounded product, and each entry of G and
 * of rho is ONE rounded product of s and the block entry (of s and the rounded difference f - f_ref).
 * idocp_rbd_objective_residual_rows returns R (0 for a NULL objective). */
int idocp_rbd_objective_residual_rows(const idocp_rbd_objective_t* o);
/* idocp_rbd_linearize_rollout_cost: what idocp_rbd_linearize_rollout takes plus an objective; step k of the rollout is step k of the objective and
 * steps <= the objective's steps.  Every output is optional (at least one is needed):
 *   A_traj, B_traj                 bit for bit what idocp_rbd_linearize_rollout writes
 *   G_traj   [steps][n][R][nz]     row-major
 *   rho_traj [steps][n][R]
 *   lx_traj  [steps + 1][n][nx], lu_traj [steps][n][nu]: the FULL gradient of `cost`: what idocp_rbd_objective_gradients defines for the diagonal
 *     terms (first_step 0, the terminal slice included) plus Gx^T rho and Gu^T rho; entry c is d_c + t_c with t_c = sum_r G[r][c] rho_r accumulated
 *     over the rows in index order by fused multiply-adds from 0.
 * With every a_weight and f_weight zero, G and rho are zero and lx, lu compare equal to the gradient call's.
 * Per step the derivative composition runs with its a, f, da_*, df_* outputs in scratch the handle owns -- it only grows, is capped at the 256 MiB of
 * the derivative call and cuts the sample axis into passes the same way --, and one launch per pass of rbd_residual_kernel.hip turns the column-major
 * blocks into the row-major scaled G, rho and G^T rho.  A sample's bits depend neither on n, nor on the outputs asked for, nor on the form of the call.
 * A non-finite input of a sample at a slice (q, v, u, contact_points, or a singular M / J M^-1 J^T) makes that sample's outputs of that slice NaN
 * and touches nothing else.  Refused: what idocp_rbd_linearize_rollout refuses, a NULL objective or io, an objective of another handle, steps beyond
 * the objective's, no output at all, u_traj NULL under a non-zero u_weight when lu_traj or lx_traj is asked for, (steps + 1) * n beyond an int (all
 * IDOCP_E_ARG), and a NEGATIVE a_weight or f_weight entry (IDOCP_E_UNSUPPORTED: a residual row needs its square root).  Task-space terms,
 * contact_distance and the constraint rows are still not differentiated (the constraint rows: idocp_rbd_linearize_rollout_penalty below). */
typedef struct idocp_rbd_cost_linearization_io {
  double *A_traj, *B_traj;      /* [steps][n][2nv*2nv], [steps][n][2nv*nu], column-major blocks */
  double *G_traj;               /* [steps][n][R][nz], row-major */
  double *rho_traj;             /* [steps][n][R] */
  double *lx_traj, *lu_traj;    /* [steps + 1][n][2nv], [steps][n][nu] */
} idocp_rbd_cost_linearization_io_t;
/* Host pointers; stages through the handle's buffer and returns when the outputs are in place. */
int idocp_rbd_linearize_rollout_cost(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                     const idocp_rbd_cost_linearization_io_t* io, int touchdown_impulse);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates only when a scratch has to grow. */
int idocp_rbd_linearize_rollout_cost_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                            double dt, const double* u_traj, const double* contact_points, const double* q_traj,
                                            const double* v_traj, const idocp_rbd_cost_linearization_io_t* io, int touchdown_impulse);

/* idocp_rbd_lqr_backward_gn: the recursion of idocp_rbd_lqr_backward on the same io, with the stage Hessian gaining G_k^T G_k, G_k = G_traj[k][i]
 * ([g_rows][nz] row-major, columns [dq | dv | du]: what the call above writes with g_rows = R):
 *   Qxx = Wx + A^T P A + Gx^T Gx,   Qux = B^T P A + Gu^T Gx,   Quu = Wu + regularization I + B^T P B + Gu^T Gu.
 * G^T G is accumulated on top of Z^T P Z, four rows of G per v_mfma_f64_16x16x4_f64 in row order.  The gradients lx, lu are the caller's (the FULL
 * ones of the call above); G enters the Hessian only.  g_rows must be a multiple of 4 within 4 .. 64, else IDOCP_E_ARG; G_traj = NULL with
 * g_rows = 0 is idocp_rbd_lqr_backward bit for bit (the same kernel is launched), G_traj = NULL with another g_rows or g_rows = 0 with a G_traj is
 * IDOCP_E_ARG.  Failure is per sample as there; a non-finite entry of G_traj[k][i] fails sample i at step k. */
int idocp_rbd_lqr_backward_gn(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_lqr_backward_gn_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj);

/* idocp_rbd_ilqr_iterate_gn: idocp_rbd_ilqr_iterate on the same io with idocp_rbd_linearize_rollout_cost_device in place of the linearisation and
 * the gradients, idocp_rbd_lqr_backward_gn_device (g_rows = R) in place of the backward pass, and the same trial rounds.  It takes any objective the
 * score takes; the diagonal weights are those of idocp_rbd_objective_lqr_weights_device (which this call reads without its refusal).  With every
 * a_weight and f_weight zero it reproduces idocp_rbd_ilqr_iterate to rounding (the sums differ: not bit for bit).  The workspace is the one of
 * idocp_rbd_ilqr_iterate with G_traj [steps][n][R][nz] carved BEHIND everything else (after done); rho is not kept. */
unsigned long long idocp_rbd_ilqr_gn_workspace_bytes(const idocp_rbd_t* h, int n, int steps);
int idocp_rbd_ilqr_iterate_gn_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);
int idocp_rbd_ilqr_iterate_gn(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                              const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);

/* ---- Constrained iLQR: the constraint rows of the objective as a squared-hinge penalty (rbd_penalty_kernel.hip, the penalty form of
 * rbd_residual_kernel.hip, the third form of rbd_lqr_kernel.hip).  ADDITIONS.  The calls above do not differentiate the constraint rows and keep
 * their refusals and their bits; the calls below do.  This is the definition.  The rows of stage k are the g_row of idocp_rbd_score_rollout,
 * h_row = max(0, g_row); the terminal slice has no rows:
 *   sq_violation[i] = sum_k dt 1/2 sum_rows h_row^2
 *   merit[i]        = cost[i] + mu sq_violation[i],   mu >= 0.
 * A lower / upper pair on one quantity x cannot both be positive when lo <= hi, so the pair is ONE signed row b = max(0, x - hi) - max(0, lo - x)
 * (a side that is switched off is left out).  The calls below refuse an enabled pair with lo > hi (IDOCP_E_ARG, idocp_last_error names the pair).
 * A row is active iff g > 0 strictly.  To the optimiser the penalty is more Gauss-Newton rows plus a diagonal; with s = sqrt(dt mu), the correctly
 * rounded root of the rounded product:
 *   dense rows, Rc = roundup4(nu + ncone ncontacts) of them, ncone = 0, 5 (LinearizedFrictionCone) or 2 (FrictionCone); 32 or 20 on the
 *   quadruped, roundup4(nu) on a chain:
 *     row j < nu, the acceleration box of actuated joint j:   sigma = s b_a[j],   Gc row = s [b != 0] [da_j/dq | da_j/dv | da_j/du]
 *     row nu + ncone c + r, contact c active at step k:       sigma = s h,        Gc row = s [g > 0] (dg/df_c) [df_c/dq | df_c/dv | df_c/du]
 *       LinearizedFrictionCone: g = (Jc f_c)_r, dg/df_c = (Jc)_r with the Jc of the score;
 *       FrictionCone: g_0 = -fz, g_1 = fx^2 + fy^2 - mu_f^2 fz^2 with dg_1/df_c = (2 fx, 2 fy, -2 mu_f^2 fz), mu_f the friction coefficient
 *     rows of kinds switched off, of inactive contacts, and the padding rows are zero;
 *   diagonal part: the q, v and u boxes of the actuated joints are diagonal in [dq; dv; du] and get no dense row --
 *     D[k][i][c] = dt mu [b != 0] at the joint's own dq, dv or du column, 0 elsewhere (the base columns are 0); the gradient gains dt mu b there.
 * The gradient of the merit is that of idocp_rbd_linearize_rollout_cost plus Gc^T sigma plus the diagonal terms.  The blocks are those of STAGE
 * mode at slice k, as for the cost rows.  Out of scope: task-space terms, contact_distance, impulse cones (multipliers: the block below).
 * idocp_rbd_objective_constraint_rows returns Rc (0 for a NULL objective and for one created with constraints == NULL). */
int idocp_rbd_objective_constraint_rows(const idocp_rbd_objective_t* o);
/* idocp_rbd_score_penalty: sq_violation [n] of the window of `steps` steps at first_step, with first_step, steps, active and accumulate as
 * idocp_rbd_score_rollout takes them; q_traj, v_traj, u_traj, a_traj, f_traj are the window's [steps][n][..] slices.  An array is read only where
 * an enabled row needs it and may be NULL otherwise; a missing array under an enabled row is IDOCP_E_ARG naming the array.  One launch.  The rows
 * of a step are folded by a fixed tree, the steps added in index order, so a sample's result is bit for bit the same whatever n is and whether it
 * was scored at once or window by window.  A non-finite entry in what is read of a sample makes its result NaN and touches no other sample.
 * Host pointers; returns when the result is in place. */
int idocp_rbd_score_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                            const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                            double* sq_violation);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_score_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                   const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                                   double* sq_violation);
/* idocp_rbd_linearize_rollout_penalty: idocp_rbd_linearize_rollout_cost plus mu.  Every output is optional (at least one is needed):
 *   A_traj, B_traj                      bit for bit the cost call's
 *   G_traj   [steps][n][R + Rc][nz]     rows 0 .. R - 1 bit for bit the cost call's G, the constraint rows behind them
 *   rho_traj [steps][n][R + Rc]         the cost call's rho, sigma behind it
 *   D_traj   [steps][n][nz]
 *   lx_traj, lu_traj                    as the cost call's, the gradient of merit: entry c is (d_c + t_c) + dt mu b_c, t_c the cost call's sum continued
 *                                       over the constraint rows in index order
 * With mu = 0, or no row switched on, the constraint rows and D are zero and lx, lu compare equal to the cost call's.  One launch per pass of the
 * penalty form of rbd_residual_kernel.hip loads the scratch blocks once and writes both kinds of rows.  An entry of a constraint row is the
 * coefficient s [active] dg/df times the block entry; a cone row sums its three products by fused multiply-adds in the order x, y, z.  NaN containment,
 * independence of n and of the outputs asked for, and the refusals are the cost call's; besides, a negative or non-finite mu and an enabled pair
 * with lo > hi are IDOCP_E_ARG. */
typedef struct idocp_rbd_penalty_linearization_io {
  double *A_traj, *B_traj;      /* [steps][n][2nv*2nv], [steps][n][2nv*nu], column-major blocks */
  double *G_traj;               /* [steps][n][R + Rc][nz], row-major */
  double *rho_traj;             /* [steps][n][R + Rc] */
  double *D_traj;               /* [steps][n][nz] */
  double *lx_traj, *lu_traj;    /* [steps + 1][n][2nv], [steps][n][nu] */
} idocp_rbd_penalty_linearization_io_t;
/* Host pointers; stages through the handle's buffer and returns when the outputs are in place. */
int idocp_rbd_linearize_rollout_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                        const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                        const idocp_rbd_penalty_linearization_io_t* io, double mu, int touchdown_impulse);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates only when a scratch has to grow. */
int idocp_rbd_linearize_rollout_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                               double dt, const double* u_traj, const double* contact_points, const double* q_traj,
                                               const double* v_traj, const idocp_rbd_penalty_linearization_io_t* io, double mu, int touchdown_impulse);

/* idocp_rbd_lqr_backward_gn_diag: idocp_rbd_lqr_backward_gn with D_traj [steps][n][nz]: Qxx and Quu gain diag(D_k) at the point where wx / wu are
 * added when H is stored -- entry (c, c) is (H + w) + D_k[c].  D_traj = NULL reproduces idocp_rbd_lqr_backward_gn bit for bit (the same kernel is
 * launched); a D_traj without a G_traj is IDOCP_E_ARG.  A negative or non-finite entry of D_traj[k][i] fails sample i at step k.  g_rows is capped
 * at 64 as there: the 32 + 32 rows of the quadruped fit exactly. */
int idocp_rbd_lqr_backward_gn_diag(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj,
                                   const double* D_traj);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_lqr_backward_gn_diag_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj,
                                          const double* D_traj);

/* idocp_rbd_ilqr_iterate_penalty: idocp_rbd_ilqr_iterate_gn on the same io, read like this: `penalty` is mu, and `violation` holds sq_violation in
 * and out (the caller scores the first rollout with idocp_rbd_score_penalty).  The chain: idocp_rbd_linearize_rollout_penalty_device;
 * idocp_rbd_lqr_backward_gn_diag_device with g_rows = R + Rc; the same trial rounds, with idocp_rbd_score_penalty_device filling the trial
 * `violation` after idocp_rbd_score_rollout_device has filled the trial cost; the unchanged idocp_rbd_ilqr_accept_device.  A sample's merit
 * therefore never rises.  An objective created with constraints == NULL has Rc = 0: D stays out, and the iteration compares equal to
 * idocp_rbd_ilqr_iterate_gn.  No host decisions on the stream.  The workspace is the one of idocp_rbd_ilqr_iterate_gn with G_traj
 * [steps][n][R + Rc][nz] and D_traj [steps][n][nz] behind it; its size depends on the objective's cone (0 for a NULL or foreign objective). */
unsigned long long idocp_rbd_ilqr_penalty_workspace_bytes(const idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps);
int idocp_rbd_ilqr_iterate_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                          double dt, const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);
int idocp_rbd_ilqr_iterate_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                   const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse);

/* ---- Augmented-Lagrangian iLQR: a first-order multiplier on every constraint row (rbd_al_kernel.hip, the AL form of rbd_residual_kernel.hip).
 * ADDITIONS.  The penalty calls above keep their refusals and their bits.  A pure penalty reaches feasibility only as mu grows without bound,
 * which ruins the conditioning of the stage Hessian; with a multiplier estimate per row mu stays moderate.  This is the definition.
 * Multiplier layout.  L = idocp_rbd_objective_multiplier_rows(o) = 4 nu + ncone ncontacts rows per (step, sample): 68 or 56 on the quadruped,
 * 4 nv on a chain, always even; 0 for a NULL objective and for one created with constraints == NULL.  Row kind nu + j, kind = 0 .. 3, is the q, v,
 * u, a box of actuated joint j; row 4 nu + ncone c + r is cone row r of contact c.  lambda_traj is [steps][n][L]; lambda_traj == NULL means all
 * zeros.  Rows of kinds switched off, and of contacts inactive at a step, are ignored on read and written as 0 by the update.
 * The shift.  Every call of this block needs mu > 0, finite (IDOCP_E_ARG otherwise).  The augmented Lagrangian of a row is the squared hinge of
 * the shifted row minus a term that does not depend on the trajectory: for g <= 0 with lambda >= 0,
 *   psi = (1 / 2 mu) (max(0, lambda + mu g)^2 - lambda^2) = (mu / 2) max(0, g + lambda / mu)^2 - lambda^2 / 2 mu,
 * and for a lower / upper pair on x with ONE signed lambda (Rockafellar's form for x in [lo, hi]) psi = (mu / 2) dist(x + lambda / mu, [lo, hi])^2
 * - lambda^2 / 2 mu.  In this order of operations, without contraction into fused multiply-adds:
 *   box:       y = x + lambda / mu (the quotient rounded, then the sum),   b~ = [upper] max(0, y - hi) - [lower] max(0, lo - y)
 *   cone row:  g~ = g + lambda / mu,  h~ = max(0, g~),  g as idocp_rbd_score_penalty computes it; the row is active iff g~ > 0, dg/df is unchanged
 *   sq_shifted[i] = sum_k dt 1/2 sum_rows b~^2 | h~^2, folded by the same tree and step order as sq_violation
 *   merit[i]      = cost[i] + mu sq_shifted[i]: the constant sum lambda^2 / 2 mu is DROPPED -- it moves no minimiser and no Armijo test, but
 *                   merits under different multipliers are not comparable
 *   update:    lambda+ = mu b~ (box, signed) or mu h~ (cone), ONE rounded product.
 * A non-finite lambda makes that sample's result NaN and touches no other sample.  A wrong-signed lambda on a one-sided row (a negative one on a
 * cone row or on an upper-only acceleration box, a positive one on a lower-only box) is NOT refused: it merely shifts the row away from its
 * bound; the update never produces one.  Still out of scope: task-space terms, contact_distance, impulse cones, latching footholds in the trial
 * rollouts. */
int idocp_rbd_objective_multiplier_rows(const idocp_rbd_objective_t* o);
/* idocp_rbd_score_al: idocp_rbd_score_penalty plus mu and the window's lambda_traj [steps][n][L]; returns sq_shifted [n].  One launch; a sample's
 * result is bit for bit independent of n and of the windowing.  With lambda_traj == NULL or all zeros it is idocp_rbd_score_penalty bit for bit. */
int idocp_rbd_score_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                       const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                       const double* lambda_traj, double* sq_shifted);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_score_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                              const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                              const double* lambda_traj, double* sq_shifted);
/* idocp_rbd_multiplier_update: on the same window, lambda_out [steps][n][L] = lambda+ (lambda_out may alias lambda_traj; needed where L > 0), and
 * two optional statistics [n]:
 *   infeasibility     = max over steps and rows of the UNSHIFTED |b| / max(0, g)
 *   multiplier_change = max over steps and rows of |lambda+ - lambda| (rows that are ignored count 0)
 * With accumulate both take the maximum with what the arrays hold (window after window); a maximum has no order, so the bits are fixed.  A
 * non-finite entry in what is read of a sample makes both statistics of the sample NaN (and keeps them NaN under accumulate) and every row of
 * lambda_out of the (step, sample) where it was read NaN.  One launch, one wavefront per sample; no atomics. */
int idocp_rbd_multiplier_update(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                                const double* lambda_traj, double* lambda_out, double* infeasibility, double* multiplier_change);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_multiplier_update_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                       const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                                       double mu, const double* lambda_traj, double* lambda_out, double* infeasibility, double* multiplier_change);
/* idocp_rbd_linearize_rollout_al: idocp_rbd_linearize_rollout_penalty plus lambda_traj [steps][n][L], into the same io.  The constraint rows of
 * G_traj and rho_traj hold sigma = s b~ | s h~ with the coefficients s [b~ != 0] and s [g~ > 0] dg/df, D = dt mu [b~ != 0], and the gradient gains
 * dt mu b~: the gradient of merit = cost + mu sq_shifted.  Everything else is the penalty call's: A, B and the cost rows bit for bit, one launch per
 * pass, NaN containment (a non-finite multiplier counts as an input of its sample for G, rho, D, lx and lu; A and B do not read it), independence of n and of the outputs asked for, the refusals
 * -- but mu = 0 is refused here.  lambda_traj == NULL or all zeros gives every output of the penalty call bit for bit. */
int idocp_rbd_linearize_rollout_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                   const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                   const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse);
/* Device pointers; asynchronous on idocp_rbd_stream(h); allocates only when a scratch has to grow. */
int idocp_rbd_linearize_rollout_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                          const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                          const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse);
/* idocp_rbd_ilqr_iterate_al: idocp_rbd_ilqr_iterate_penalty plus lambda_traj [steps][n][L] (NULL: zeros; then it is that call bit for bit).
 * `penalty` of io is mu (> 0), `violation` holds sq_shifted in and out.  The chain: idocp_rbd_linearize_rollout_al_device; the unchanged
 * idocp_rbd_lqr_backward_gn_diag_device; the trial rounds with idocp_rbd_score_al_device filling the trial `violation`; the unchanged
 * idocp_rbd_ilqr_accept_device.  A sample's cost + mu sq_shifted never rises while lambda and mu stay.  The workspace is the one of
 * idocp_rbd_ilqr_penalty_workspace_bytes.  No host decisions on the stream.  The multipliers are read, never written. */
int idocp_rbd_ilqr_iterate_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda_traj, int touchdown_impulse);
int idocp_rbd_ilqr_iterate_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                              const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda_traj, int touchdown_impulse);
/* idocp_rbd_ilqr_al_update: the outer step on the current rollout (q_traj, v_traj, u_traj, a_traj, f_traj as idocp_rbd_ilqr_io_t holds them; the
 * `steps` stage slices are read).  lambda_traj [steps][n][L] becomes lambda+ under mu, IN PLACE; then violation [n] = sq_shifted under lambda+ and
 * mu_next, so that the next iteration's acceptance test has a consistent baseline; infeasibility and multiplier_change [n] (either may be NULL)
 * are the statistics of idocp_rbd_multiplier_update over all steps.  Beyond IDOCP_RBD_SCORE_MAX_WINDOW steps both passes go window by window.
 * The schedule of mu (mu_next = mu keeps it) stays with the caller.  Host pointers; returns when the results are in place. */
int idocp_rbd_ilqr_al_update(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, const double* q_traj,
                             const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu, double mu_next,
                             double* lambda_traj, double* violation, double* infeasibility, double* multiplier_change);
/* Device pointers, asynchronous on idocp_rbd_stream(h); allocates nothing. */
int idocp_rbd_ilqr_al_update_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, const double* q_traj,
                                    const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu, double mu_next,
                                    double* lambda_traj, double* violation, double* infeasibility, double* multiplier_change);

/* ---- Sampling around a torque sequence: perturb, weigh, average (rbd_sample_kernel.hip).  Every call of this block is an ADDITION (the reference
 * has no counterpart).  With idocp_rbd_rollout_policy_device and idocp_rbd_score_rollout_device between the first and the second, one iteration of
 * a sampling-based refinement (the MPPI update: the softmin-weighted mean of the sampled torque sequences) runs on the handle's stream without a
 * synchronisation.  Both model kinds work; only nu matters.
 * Every sum over the sample axis is folded in a FIXED order: partial sums over chunks of IDOCP_RBD_REDUCE_CHUNK consecutive samples (within a
 * chunk: each of 256 lanes adds its samples in index order, then a fixed tree over the lanes), then the chunks in index order.  No floating-point
 * atomics.  Results are therefore bit for bit equal from run to run and between the host and the device form, and a row of
 * idocp_rbd_weighted_mean depends neither on `rows` nor on the call that carried it.
 * The chunk partials live in one more buffer the handle owns; it grows only when rows * ceil(n / IDOCP_RBD_REDUCE_CHUNK) grows (rows = 1 for
 * idocp_rbd_importance_weights). */
#define IDOCP_RBD_REDUCE_CHUNK 1024
#define IDOCP_RBD_WEIGHT_STATS 5
#define IDOCP_RBD_MEAN_MAX_COLUMNS 64

/* ADDITION.  u_samples[k][i][j] = clamp(u_nominal[k][j] + sigma[j] z(seed, draw, first_step + k, i, j)) for k < steps, i < n, j < nu, with
 * u_nominal [steps][nu], sigma [nu], u_min / u_max [nu] (either may be NULL) and the clamp min(max(u, u_min), u_max) of the policy.
 * z = 0 exactly for sample 0: the nominal itself is always among the candidates.  Otherwise z is a standard normal from Philox4x32-10 (multipliers
 * 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with the key (seed low word, seed high word) and the counter
 * (i, first_step + k, j / 2, draw); of its output words r0 .. r3
 *   u1 = (((r0 | r1 << 32) >> 12) + 0.5) 2^-52 in (0, 1),  u2 = ((r2 | r3 << 32) >> 11) 2^-53 in [0, 1),  rho = sqrt(-2 ln u1),
 * an even j takes rho cos(2 pi u2) and an odd j rho sin(2 pi u2); |z| <= sqrt(106 ln 2) = 8.57.  draw is the caller's iteration counter: a new
 * value gives fresh noise.  A sample's values depend on (seed, draw, step, i, j) alone: they are bit for bit the same whatever n is and whether
 * the steps came in one call or window by window (first_step).  n >= 1, first_step >= 0, steps >= 1.
 * Host pointers; returns when u_samples is in place.  Refuses (IDOCP_E_ARG) a sigma that is negative or not finite, and bounds like
 * idocp_rbd_feedback_torques_batch. */
int idocp_rbd_perturb_torques(idocp_rbd_t* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma, const double* u_min,
                              const double* u_max, unsigned long long seed, unsigned draw, double* u_samples);
/* Device pointers for everything; asynchronous on idocp_rbd_stream(h); one launch; allocates nothing.  sigma and the bounds are NOT checked. */
int idocp_rbd_perturb_torques_device(idocp_rbd_t* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma,
                                     const double* u_min, const double* u_max, unsigned long long seed, unsigned draw, double* u_samples);

/* ADDITION.  The softmin importance weights of n scores s_i = cost[i] + penalty violation[i] (violation NULL: s_i = cost[i]).  F = the samples whose
 * s_i is finite (a diverged plant scores NaN), s_min = min over F:
 *   weights[i] = exp(-(s_i - s_min) / temperature) on F, exactly 0 elsewhere
 * so the best sample weighs exactly 1 and W = sum_i weights[i] >= 1 unless F is empty.  stats [IDOCP_RBD_WEIGHT_STATS] = {|F|, s_min, the argmin
 * (the lowest index at a tie), W, the effective sample size W^2 / sum_i weights[i]^2}; with F empty all weights are 0 and stats = {0, NaN, -1, 0, 0}.
 * temperature finite and positive, penalty finite and non-negative, else IDOCP_E_ARG (in both forms).
 * Host pointers; returns when weights and stats are in place. */
int idocp_rbd_importance_weights(idocp_rbd_t* h, int n, const double* cost, const double* violation, double penalty, double temperature,
                                 double* weights, double* stats);
/* Device pointers, stats included; asynchronous on idocp_rbd_stream(h); four launches; allocates only when ceil(n / IDOCP_RBD_REDUCE_CHUNK) grows
 * beyond what any earlier call of this block needed. */
int idocp_rbd_importance_weights_device(idocp_rbd_t* h, int n, const double* cost, const double* violation, double penalty, double temperature,
                                        double* weights, double* stats);

/* ADDITION.  The weighted mean over the sample axis of a step-major array x [rows][n][m], 1 <= m <= IDOCP_RBD_MEAN_MAX_COLUMNS (nu, nv, nq and
 * 3 ncontacts fit: u_traj, q_traj, f_traj ... of a rollout can be passed straight in), rows >= 1:
 *   mean[r][c] = sum_i weights[i] x[r][i][c] / sum_i weights[i]
 * A sample with weights[i] == 0 is SKIPPED, not multiplied: its x may hold NaN or Inf (what a diverged rollout leaves) without touching the
 * result.  A non-finite x under a positive weight makes exactly the entries mean[r][c] it enters non-finite.  sum_i weights[i] == 0 gives NaN
 * everywhere (read stats[0] of the call above first).
 * Host pointers; returns when mean is in place.  Refuses (IDOCP_E_ARG) a weight that is negative or not finite. */
int idocp_rbd_weighted_mean(idocp_rbd_t* h, int n, int rows, int m, const double* weights, const double* x, double* mean);
/* Device pointers; asynchronous on idocp_rbd_stream(h); two launches (the chunk partials, then the fold and the division); the weights are NOT
 * checked; allocates only when rows * ceil(n / IDOCP_RBD_REDUCE_CHUNK) grows beyond what any earlier call of this block needed.  mean may lie
 * anywhere outside x and weights -- e.g. be the u_nominal of the next idocp_rbd_perturb_torques_device. */
int idocp_rbd_weighted_mean_device(idocp_rbd_t* h, int n, int rows, int m, const double* weights, const double* x, double* mean);

const char* idocp_last_error(void);
const char* idocp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* IDOCP_HIP_H_ */
