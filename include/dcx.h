/*
 * dcx.h — C ABI of libdcx.so, the MI355X (gfx950) implementation of DiffCo's
 * score(+gradient) hot path.
 *
 * The reference (ucsdarclab/diffco) has no FFI: its boundary for this path is a set of
 * Python call signatures.  Each entry point below names the reference code it replaces
 * (paths under /root/reference).  Signatures use only plain pointers and sizes — no torch
 * types — so any host (ctypes, cgo, JNI, a C++ planner) can bind them; see INTEGRATION.md.
 *
 * Conventions
 *   - All arrays are dense, row-major, fp32.  "dev" = device pointer on the model's GPU,
 *     "host|dev" = either (copied with hipMemcpyDefault at create time).
 *   - The caller owns every q/score/grad/jac buffer.  The library owns only the model's
 *     device copy of the support rows and FK parameters (freed by dcx_model_destroy).
 *   - Every launch is enqueued on the caller's HIP stream (`stream` = hipStream_t, NULL =
 *     default stream) and does NOT synchronise.
 *   - Return value: 0 = DCX_OK, otherwise an error code; text via dcx_last_error()
 *     (thread-local).  Nothing throws or exits across the ABI.
 *   - A model handle's numerical state is immutable after creation: concurrent calls on distinct
 *     streams are legal (small-batch launches keep one internal scratch buffer per stream, allocated on
 *     the stream's first small-batch call and freed only by dcx_model_destroy).  A HIP graph captured
 *     from these calls holds that buffer: keep the model alive while the graph exists, and replay the
 *     graph on the stream it was captured on (or at least never concurrently with other small-batch
 *     calls of the same model on the capture stream — they share the buffer's arrival counters).
 */
#ifndef DCX_H
#define DCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCX_VERSION 109 /* 0.1.8: the optimisers' collision term for several classes under per-class margins (dcx_score_hinge_grad_mc, dcx_traj_adam_run_mc, dcx_traj_adam_step_mc), dcx_dh_frames / dcx_euler_frames (utils.DH2mat / euler2mat); 0.1.7: dcx_escape_adam (the escape loop of scripts/escape.py on the stream); 0.1.6: dcx_debug_clock_probe; the matrix-core forms left the default build (since removed: dcx_debug_set("mfma" / "xm", 1) -> DCX_ERR_UNSUPPORTED); owner-polls words tagged per launch, give-up reported by the model's next launch; 0.1.5: dcx_model_create_ex / dcx_model_update (rows packed on the device); 0.1.4: dcx_train_perceptron_ex (per-call flags); 0.1.3: dcx_fk_desc carries the DCX_FK_TREE section; 32 control points, D <= 96 */

/* ---- status codes ---------------------------------------------------------------- */
#define DCX_OK 0
#define DCX_ERR_INVALID 1     /* bad argument (NULL, negative size, inconsistent shapes) */
#define DCX_ERR_UNSUPPORTED 2 /* shape/kind outside the compiled set (e.g. D > DCX_MAX_D) */
#define DCX_ERR_HIP 3         /* a HIP runtime call failed (message has hipGetErrorString) */
#define DCX_ERR_NO_DEVICE 4   /* no gfx950 device visible */

/* ---- pairwise kernel functions (diffco/kernel.py) -------------------------------- */
/* K(x, s) as a function of d2 = ||x - s||^2, r = sqrt(d2); kparams = {p0, p1}.        */
#define DCX_K_RQ 0   /* RQKernel       kernel.py:12-29   (1 + p0/p1 * d2)^(-p1); p0=gamma, p1=p */
#define DCX_K_POLY 1 /* Polyharmonic   kernel.py:59-79   p0=k, p1=eps: k odd r^k/eps; k even r^k log r/eps (0 at r=0) */
#define DCX_K_MQ 2   /* MultiQuadratic kernel.py:45-57   sqrt(d2/p0^2 + 1); p0=eps */

/* ---- forward-kinematics transforms (diffco/model.py == diffco/robot_fkine.py) ---- */
#define DCX_FK_NONE 0   /* transform=None: features are the configuration itself (D = dof)      */
#define DCX_FK_PLANAR 1 /* RevolutePlanarRobot.fkine      model.py:40-48                        */
#define DCX_FK_DH 2     /* DH chains: Baxter L/R model.py:225-241,283-299; BaxterDual 366-383;
                           PandaFK 430-453 (robot_fkine.py:428-444); DualPandaFK 486-502;
                           link transform = utils.DH2mat utils.py:66-75                        */
#define DCX_FK_SE2 3    /* RigidPlanarBody.fkine          model.py:90-93 (utils.rot_2d)         */
#define DCX_FK_SE3 4    /* RigidBody.fkine                model.py:156-159 (utils.euler2mat = Rz Ry Rx) */
#define DCX_FK_TREE 5   /* URDF kinematic tree, flattened into root-to-leaf chains: link-origin features of
                           RobotDiffCo.tensorized_fkine_single_robot collision_checkers.py:385-393 over
                           URDFRobot.compute_forward_kinematics_all_links urdf_interface.py:516-553 and
                           RigidBody.forward_kinematics collision_interfaces/rigid_body.py:82-140      */

/* joint motions of DCX_FK_TREE (rigid_body.py:100-126); the joint variable is v = t_scale * q + t_offset */
#define DCX_J_FIXED 0     /* no motion (fixed joints that were not merged into their successor)        */
#define DCX_J_REV_X 1     /* x_rot(v)  spatial_vector_algebra.py x_rot                                  */
#define DCX_J_REV_Y 2     /* y_rot(v)                                                                    */
#define DCX_J_REV_Z 3     /* z_rot(v)                                                                    */
#define DCX_J_PRISMATIC 4 /* translation t_axis * v along the joint's own (post-fixed-transform) axes   */

#define DCX_MAX_JOINTS 16 /* per chain */
#define DCX_MAX_CHAINS 2
#define DCX_MAX_POINTS 32
#define DCX_MAX_DOF 32
#define DCX_MAX_D 96  /* feature width n_points * point_dim the fused kernels are compiled for */
#define DCX_MAX_C 8   /* weight columns (classes) the fused kernels are compiled for           */
#define DCX_MAX_TREE_CHAINS 16 /* root-to-leaf paths of a DCX_FK_TREE                           */
#define DCX_MAX_TREE_BASES 4   /* distinct base transforms among them (robots side by side)     */
#define DCX_MAX_TREE_JOINTS 64 /* joints summed over all paths (shared prefixes count per path) */

/*
 * Plain-data description of one `transform(q[dof]) -> control points [n_points, point_dim]`.
 * Output feature k*point_dim + j is coordinate j of control point k, i.e. the row-major
 * flattening the reference kernels apply (kernel.py:20-21, 77).
 */
typedef struct dcx_fk_desc {
    int32_t kind;      /* DCX_FK_*                                                          */
    int32_t dof;       /* width of a configuration row                                      */
    int32_t n_points;  /* m (for DCX_FK_NONE: dof)                                          */
    int32_t point_dim; /* d = 2 or 3 (for DCX_FK_NONE: 1)                                   */

    /* DCX_FK_PLANAR: phi_i = sum_{j<=i} q_j; p_i = sum_{j<=i} l_j (cos phi_j, sin phi_j)   */
    float link_length[DCX_MAX_DOF];

    /* DCX_FK_DH: n_chains serial chains.  Joint i of chain c reads q[joint_q[c][i]], adds
     * theta0, and applies T <- T * DH(theta, a, d, sin_alpha, cos_alpha) starting from
     * base[c] (row-major 3x4 [R|t]).  Control point k is base-frame position of
     * pt_off[k] expressed in frame pt_frame[k] (0-based joint index, i.e. after joint
     * pt_frame[k]'s transform) of chain pt_chain[k].                                      */
    int32_t n_chains;
    int32_t chain_len[DCX_MAX_CHAINS];
    int32_t joint_q[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float a[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float d[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float sin_alpha[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float cos_alpha[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float theta0[DCX_MAX_CHAINS][DCX_MAX_JOINTS];
    float base[DCX_MAX_CHAINS][12];
    int32_t pt_chain[DCX_MAX_POINTS];
    int32_t pt_frame[DCX_MAX_POINTS];
    float pt_off[DCX_MAX_POINTS][3];

    /* DCX_FK_SE2: q = (x, y, theta); p_k = R(theta) keypoints[k][0:2] + (x, y)
     * DCX_FK_SE3: q = (x, y, z, roll, pitch, yaw); p_k = Rz(yaw) Ry(pitch) Rx(roll) keypoints[k] + (x,y,z) */
    float keypoints[DCX_MAX_POINTS][3];

    /* DCX_FK_TREE: t_n_chains serial chains stored back to back in the t_* joint arrays (chain c owns the
     * next t_chain_len[c] entries).  A chain starts from t_base[c] (row-major 3x4) and every joint applies
     *     T <- T * [t_fixed | as 3x4] * Motion(t_type, t_scale * q[t_q] + t_offset)
     * i.e. the joint's <origin> followed by its motion, as rigid_body.py:100-126 composes them.  A URDF
     * tree becomes one chain per leaf; joints on a shared prefix are simply repeated (the library merges
     * identical prefixes back into one node when it compiles the description, so they are computed once).  Mimic joints use the driver's t_q with the mimic multiplier/offset
     * (rigid_body.py:93-94); an axis of -1 is a negative t_scale (rigid_body.py:103-108).
     * Control point k is pt_off[k] in the frame after joint pt_frame[k] (index within its chain) of chain
     * pt_chain[k].  t_coord_major != 0 lays the features out as [3][n_points] (feature j*n_points + k), the
     * torch.stack(..., dim=-1) layout of collision_checkers.py:390; 0 keeps [n_points][3].               */
    int32_t t_n_chains;
    int32_t t_coord_major;
    int32_t t_chain_len[DCX_MAX_TREE_CHAINS];
    float t_base[DCX_MAX_TREE_CHAINS][12];
    int32_t t_type[DCX_MAX_TREE_JOINTS];
    int32_t t_q[DCX_MAX_TREE_JOINTS];
    float t_scale[DCX_MAX_TREE_JOINTS];
    float t_offset[DCX_MAX_TREE_JOINTS];
    float t_fixed[DCX_MAX_TREE_JOINTS][12];
    float t_axis[DCX_MAX_TREE_JOINTS][3];
} dcx_fk_desc;

typedef struct dcx_model dcx_model; /* opaque; changed only by dcx_model_update */

/* ---- library ----------------------------------------------------------------------- */
int dcx_version(void);
const char* dcx_last_error(void);
int dcx_device_count(void);

/* Developer knobs for tests and A/B tools: override one of the launch-geometry rules (they change how the work
 * is split over blocks, never what is computed).  name: "ys" (support super-chunks per tile), "nw" (waves per
 * block), "min_rows" (supports per wave slice), "split_finish_kernel" (1 = finish split launches with a second
 * launch), "inlaunch_tiles", "jac_per_class" (1 = one launch per class in dcx_score_jac), "mfma" and "xm" (the
 * matrix-core forms, removed: 0 and rule are accepted, 1 answers DCX_ERR_UNSUPPORTED), "xf" (0 = the sweep in its direct form everywhere, 1 / rule =
 * the expanded form wherever it is compiled and the model qualifies: Polyharmonic(1), or RQKernel(p = 2) behind an FK
 * transform with gamma * max |s - centroid|^2 <= 32; rows of <= 37 floats; the two forms agree to ~1e-6; 2 = also for RQ
 * models outside that rule: measurements only),
 * "traj_fused" (0 = dcx_traj_adam_run as two launches per iteration), "jac_one_sweep" (0 = dcx_score_jac never takes the
 * one-sweep kernel, 1 = whenever it is compiled and the batch is beyond the one-launch-per-all-classes regime),
 * "train_grid" (see dcx_train_perceptron), "fkk" (which FK walk a DH arm takes: 2 / rule = the step table, 1 = the FK
 * program through scalar loads, 0 = the FK program from its LDS copy; bit-identical results), "jt_waves" (0 = the chain and
 * J^T phases of a DH arm on one wave instead of several; bit-identical), "traj_ys" (workgroups per path of the persistent
 * trajectory kernel: 1 = one, k = k; rule = what fills the chip, at most 8), "traj_across" (1 = a path's workgroups dealt
 * across XCDs instead of onto one: a measurement), "owner_poll" (the split launch's hand-over: 0 = arrival counters, last
 * block to arrive finishes; 1 / rule = block y = 0 owns its tile and polls its peers' (value, tag) words - bit-identical;
 * the rule takes it when every block of the launch is resident at once), "hess_ys" (blocks per tile of dcx_score_hess; 1 =
 * never split the supports), "hess_form" (dcx_score_hess: 0 = one lane per (configuration, direction) sweeps the supports, 1 = the
 * moments form - one lane per configuration sweeps gradient, coefficient sum and the symmetric D x D matrix, the direction lanes
 * read M dx - wherever it is compiled (D <= 16); rule = from B = 1024; same Hessian to fp32 round-off),
 * "motion_early_exit" (0 = dcx_check_motions sweeps every tile, none skipped behind a first hit: a measurement; same answers),
 * "solve_threads" (dcx_solve's workgroup size: 256 or 512; rule = 256 up to 736 unknowns; same pivots, same arithmetic),
 * "qt" (small batches of a one-class D = 12 / 24 model as tiles of 16 configurations that sweep all the rows from an LDS copy
 * instead of the split launch: 0 = never, 1 = wherever it is compiled and fits with >= 4 waves; rule = at most 16
 * configurations per CU and room for all 16 waves, unless another knob asks for a particular form of the launch).
 * "skew" (how a 16-wave block's rows are dealt to its four wave groups: 0 = equal slices, w0 | w1 << 10 | w2 << 20 = the per-mille
 * shares of groups 0 - 2, rule = 480 / 320 / 150 / 50: a SIMD issues oldest-first and a block's last waves would finish alone; the tile of 16 configurations
 * deals its row slices the same way), "skew8" (the same for 8-wave blocks: the per-mille share of waves 0 - 3, rule = 600, 0 = equal).
 * "knn_split" (dcx_knn's point splits: n > 0 = n blocks per query tile, at most 1024, 0 / rule = what the plan picks;
 * dcx_knn_work_bytes follows the knob; bit-identical results).
 * value < 0 restores the rule.  The initial values come from the DCX_YS / DCX_NW / DCX_XF / ... environment variables,
 * read once at library load; no launch calls getenv.   */
int dcx_debug_set(const char* name, int64_t value);
/* Measurement aid (0.1.6): one wave on `stream` samples the shader clock counter (s_memtime) and the fixed-rate wall clock
 * (s_memrealtime; its rate in kHz -> *wall_clock_khz, may be NULL) when it starts and again after `wall_ticks` of the latter:
 * out4 [4] uint64 on the device = {clock0, clock1, wall0, wall1}.  (clock1 - clock0) / (wall1 - wall0) x rate = the clock the
 * shaders had meanwhile: launched beside a loop of sweeps on another stream it tells what clock the sweep ran at (under its
 * fp32-VALU load the part holds ~1.45 GHz, not its nominal 2.4: profiles/r05_clock_under_load.txt; bench.py `roofline.clock`). */
int dcx_debug_clock_probe(int device, uint64_t* out4, uint64_t wall_ticks, int32_t* wall_clock_khz, void* stream);

/* ---- model = inference state of a kernel perceptron ------------------------------- */
/* Replaces the state DiffCo.score/poly_score read: support_transformed[S,m,d] + gains[S]
 * or rbf_nodes[S] (kernel_perceptrons.py:41-53, 143-196, 282-283); old API support_fkine[S,D]
 * + rbf_nodes[S,C] (deprecated/MultiDiffCo.py:125-154).
 *   fk            NULL or kind DCX_FK_NONE => D must equal the configuration width.
 *   support_feat  [S, D]  transformed supports (already through the FK), host|dev
 *   weights       [S, C]  gains / rbf_nodes, host|dev; rows whose C weights are all zero
 *                         are dropped (they contribute nothing; this is what
 *                         max_num_supports padding produces, kernel_perceptrons.py:159-196)
 */
int dcx_model_create(dcx_model** out, int device, const dcx_fk_desc* fk, int kernel_kind,
                     const float* kparams, const float* support_feat, const float* weights,
                     int64_t S, int32_t D, int32_t C);
/* The same on a stream, with room to grow (round 4).  When support_feat and weights are DEVICE pointers the rows are packed
 * by one kernel on `stream` (dropping zero rows, folding the kernel's constants, building the centred copy) and 16 bytes
 * come back - no bulk copy through the host; `stream` is synchronised for that read-back (the number of kept rows decides
 * the launch geometry of every later call).  Host pointers take the host path.  capacity >= S reserves storage so that
 * dcx_model_update can refill the model in place (0 = exactly S).  Results are bit-identical to dcx_model_create's. */
int dcx_model_create_ex(dcx_model** out, int device, const dcx_fk_desc* fk, int kernel_kind,
                        const float* kparams, const float* support_feat, const float* weights,
                        int64_t S, int32_t D, int32_t C, int64_t capacity, void* stream);
/* New supports / weights for an existing model (same transform, kernel, D, C): what DiffCo.train / fit_poly / update do to
 * the state every round of the reference's active-learning loop (collision_checkers.py:220-252).  Reuses the model's
 * storage when S <= its capacity (else reallocates after a device synchronisation) and every per-stream scratch buffer.
 * The model must not be in use by launches on OTHER streams or threads while it is updated; launches enqueued earlier on
 * `stream` are ordered before the refill, later ones see the new rows.                                               */
int dcx_model_update(dcx_model* m, const float* support_feat, const float* weights, int64_t S, void* stream);
void dcx_model_destroy(dcx_model* m);
/* any out pointer may be NULL; S_active = supports kept after dropping all-zero rows */
int dcx_model_info(const dcx_model* m, int64_t* S_active, int32_t* D, int32_t* C, int32_t* dof,
                   int32_t* device);

/* ---- the hot path ------------------------------------------------------------------ */
/* score[b, c] = sum_j K(T(q_b), support_j) * weights[j, c]
 * Replaces DiffCo.score/score_original kernel_perceptrons.py:359-370, DiffCo.poly_score :309-319,
 * MultiDiffCo.score / rbf_score deprecated/MultiDiffCo.py:118-123,156-169, DiffCoBeta.rbf_score
 * deprecated/DiffCoBeta.py:173-181.   q [B, dof] dev -> score [B, C] dev.                 */
int dcx_score(const dcx_model* m, const float* q, int64_t B, float* score, void* stream);

/* score as above and grad[b, :] = d( sum_c upstream[b,c] * score[b,c] ) / d q_b, in the same
 * pass (the reference obtains it by autograd: optim.py:101, 211-216).  upstream [B, C] dev or
 * NULL (= all ones).  score may be NULL.  grad [B, dof] dev.                              */
int dcx_score_grad(const dcx_model* m, const float* q, int64_t B, const float* upstream,
                   float* score, float* grad, void* stream);

/* score and the full Jacobian jac[b, c, :] = d score[b,c] / d q_b  ([B, C, dof] dev)
 * (torch.autograd.functional.jacobian callers, optim.py:211-216).                          */
int dcx_score_jac(const dcx_model* m, const float* q, int64_t B, float* score, float* jac,
                  void* stream);

/* Second derivatives: hess[b, i, k] = d2( sum_c upstream[b,c] * score[b,c] ) / d q_b[i] d q_b[k]   ([B, dof, dof] dev),
 * analytic (forward-mode tangents through the FK, the sweep and the reverse FK sweep: hess_kernel.hip) — what the
 * reference obtains by a double backward through dist_est for trust-constr's constraint Hessian (optim.py:380-391,
 * torch.autograd.functional.hessian).  upstream [B, C] dev or NULL (= all ones); grad [B, dof] dev or NULL receives
 * the gradient of the same function.  A configuration that sits exactly on a support (|x - s| = 0) takes no
 * contribution from that support for Polyharmonic kernels (the kernel is not twice differentiable there).
 * Every transform kind is accepted (a tree whose frames do not fit the LDS as (value, tangent) pairs keeps them in
 * stream-ordered global scratch); a batch of a few hundred points splits the supports across blocks like
 * dcx_score_grad does.  DCX_ERR_UNSUPPORTED only if one feature row in duals exceeds a block's LDS.                */
int dcx_score_hess(const dcx_model* m, const float* q, int64_t B, const float* upstream, float* grad, float* hess,
                   void* stream);

/* score as above (C == 1 models only) and the gradient of the hinge penalty the optimisers build on it:
 *   grad[b, :] = weight * 1[score_b - margin > 0] * d score_b / d q_b
 * i.e. d/dq of  weight * clamp(dist_est(q) - safety_margin, min=0).sum()  (optim.py:88-89, 97-101) in the
 * same pass that produces the score.  score may be NULL.                                                */
int dcx_score_hinge_grad(const dcx_model* m, const float* q, int64_t B, float margin, float weight,
                         float* score, float* grad, void* stream);
/* The same for ANY class count under per-class margins - the collision term the reference's Adam loops build on a
 * MultiDiffCo score (optim.py:88-89 with options['safety_margin'] a [C] tensor: scripts/2d_trajopt.py:94-102,
 * scripts/active.py:35, 65):
 *   grad[b, :] = d/dq_b of  weight * sum_c clamp(score[b, c] - margin[c], min=0)
 *              = weight * sum_c 1[score[b, c] - margin[c] > 0] * d score[b, c] / d q_b
 * margin: C HOST floats (they travel as kernel arguments).  score [B, C] dev out; with C > 1 it must not be NULL: the
 * class scores are swept first (the hinge's upstream is only known once every support has been seen), then the gradient
 * with that upstream - two launches, no synchronisation.  C == 1 is dcx_score_hinge_grad's single launch.          */
int dcx_score_hinge_grad_mc(const dcx_model* m, const float* q, int64_t B, const float* margin, float weight,
                            float* score, float* grad, void* stream);

/* ---- fused Adam trajectory step (caller of the path) ------------------------------- */
/* Batched restatement of the loop body of adam_traj_optimize (optim.py:86-127): R independent paths of W
 * waypoints are advanced by ONE Adam step on
 *   loss = w_diff * sum |cp[w+1]-cp[w]|^2 + w_collision * sum clamp(score - margin, 0)
 *        + w_max_move * sum_{segments, points} clamp(|cp[w+1]-cp[w]|^2 - max_speed^2, 0)
 *        + w_joint_limit * sum (clamp(lo - q, 0) + clamp(q - hi, 0))
 * with the endpoints' gradient zeroed, plus the reference's bookkeeping (lowest-loss path, best valid path,
 * per-path stop when constraint <= valid_tol and |grad| < grad_tol).  All pointers are device memory owned by
 * the caller; every array is dense fp32 unless noted.                                                    */
typedef struct dcx_traj_state {
    int32_t n_paths, n_waypoints;      /* R, W (W <= 1024, and ceil(W / 64) x 64 waypoints' rows, features (twice) and FK
                                        * frames within a CU's 160 KB of LDS: DCX_ERR_UNSUPPORTED otherwise, before any launch) */
    float* path;                       /* [R, W, dof]  in/out                                            */
    float* adam_m;                     /* [R, W, dof]  first moment  (zero before step 1)                */
    float* adam_v;                     /* [R, W, dof]  second moment (zero before step 1)                */
    const float* limits;               /* [dof, 2]     joint limits (lo, hi)                             */
    const float* col_score;            /* [R*W] ([R*W, C] for the _mc entry points) dist_est(path) of THIS step */
    const float* col_grad;             /* [R*W, dof]   hinge gradient of this step (dcx_score_hinge_grad)*/
    float* stats;                      /* [R, 8] out: loss, objective, constraint, |grad|, collision, max_move, joint_limit, 0 */
    float* lowest_loss;                /* [R] in/out (+inf before step 1)                                */
    float* lowest_obj;                 /* [R] out: objective at the lowest-loss step                     */
    float* lowest_path;                /* [R, W, dof] out: path AFTER the lowest-loss step               */
    float* best_valid_obj;             /* [R] in/out (+inf before step 1)                                */
    float* best_valid_path;            /* [R, W, dof] out: path AFTER the best valid step                */
    int32_t* done;                     /* [R] in/out: 1 = path stopped (frozen); 0 before step 1         */
    int32_t* steps;                    /* [R] in/out: steps actually taken                               */
} dcx_traj_state;

typedef struct dcx_traj_opts {
    float lr, beta1, beta2, eps;       /* torch.optim.Adam defaults: beta 0.9 / 0.999, eps 1e-8          */
    float w_diff, w_collision, w_max_move, w_joint_limit; /* 1, 10, 10, 10 in the reference (optim.py:19-22) */
    float safety_margin, max_speed;
    float valid_tol, grad_tol;         /* 1e-2, 1e-4 (optim.py:114, 126)                                  */
} dcx_traj_opts;

/* one Adam step; `step` is 1-based (bias correction).  col_score / col_grad must already hold this step's
 * collision term for the CURRENT path.                                                                   */
int dcx_traj_adam_step(int device, const dcx_fk_desc* fk, const dcx_traj_state* st, const dcx_traj_opts* opt,
                       int32_t step, void* stream);
/* n_iters iterations of {dcx_score_hinge_grad(model, path) -> dcx_traj_adam_step} enqueued back to back from
 * native code, starting at 1-based step `first_step`; `model` must be a C == 1 model whose transform is the
 * robot's FK.  st->col_score / st->col_grad are used as scratch ([R*W], [R*W, dof], non-const here).      */
int dcx_traj_adam_run(const dcx_model* model, const dcx_traj_state* st, const dcx_traj_opts* opt,
                      int32_t first_step, int32_t n_iters, void* stream);
/* The same loop on a model with ANY class count C (a MultiDiffCo score) under per-class margins:
 *   collision term = sum over waypoints and classes of clamp(score[w, c] - margin[c], 0)    (optim.py:88-89 with a [C] margin)
 * margin: C HOST floats, or NULL = opt->safety_margin for every class.  st->col_score is [R*W, C] here (scratch).
 * One persistent launch per <= 192 iterations where the two-sweep form of the trajectory kernel is compiled (D <= 24,
 * RQKernel(p = 2) / Polyharmonic(1), W <= 64), else three launches per iteration (class scores, hinge-gradient sweep,
 * step); the same arithmetic either way.  dcx_traj_adam_step_mc is the step half on its own: col_score [R*W, C] and
 * col_grad [R*W, dof] must hold dcx_score_hinge_grad_mc's outputs for the current path.                            */
int dcx_traj_adam_run_mc(const dcx_model* model, const dcx_traj_state* st, const dcx_traj_opts* opt, const float* margin,
                         int32_t first_step, int32_t n_iters, void* stream);
int dcx_traj_adam_step_mc(int device, const dcx_fk_desc* fk, const dcx_traj_state* st, const dcx_traj_opts* opt,
                          const float* margin, int32_t C, int32_t step, void* stream);

/* ---- escape from collision (caller of the path; SURVEY.md §8f-2 names it beside the trajectory step) -- */
/* Batched restatement of OptimSampler.optim_escape (scripts/escape.py:19-38): Adam on the configurations themselves,
 *   for step in range(n_steps):
 *       excess = sum(dist_est(q) - safety_margin)          # escape.py:26 (no clamp: the loop stops instead)
 *       if excess <= 0: break                              # :27-28
 *       [record q]; q <- Adam(q, d excess / d q); q <- post_transform(q)       # :29-36
 * entirely on the caller's stream: per step one fused score + gradient sweep (the gradient of sum_c score_c: the
 * margin is a constant) and one update launch; nothing is read back, the loop's decisions stay on the device.
 *   joint != 0: ONE loop for the whole batch, as the reference runs it - `excess` is the sum over all B configurations
 *               and all classes, and everybody stops together;  steps [1, 2]
 *   joint == 0: B independent loops advanced together - a configuration stops (and is left where it is) as soon as its
 *               own sum over the classes is <= 0;  steps [B, 2]
 * steps (int32, device, out): per loop (evaluations of dist_est = the reference's second return value, escape.py:38;
 *   Adam steps taken - one fewer when the loop stopped on its last evaluation).
 * history (device, out, may be NULL): [n_slots, B, dof] with n_slots = (record_freq > 0 ? ceil(n_steps / record_freq) : 0)
 *   + 1: slot s / record_freq holds q BEFORE the update of step s when record_freq divides s (escape.py:29-30), and the
 *   slot behind a loop's last record its final configuration (:37); later slots are not written.  q [B, dof] is advanced
 *   in place and holds the final configurations either way.
 * margin [C] device (NULL = 0).  wrap_mask bit i: coordinate i is wrapped to [-pi, pi) after every step - all ones below
 *   dof for post_transform = utils.wrap2pi (utils.py:51-52), bit 2 for utils.se2_wrap2pi (:54-55), 0 for None.
 * work: dcx_escape_work_bytes(model, B) bytes of device memory, the caller's (Adam moments, score and gradient of the
 *   current step, the list of the loops still running); initialised here.  No allocation.
 * compact_every = 0: no synchronisation either - every step sweeps all B configurations, stopped loops included (they are
 *   left alone by the update), and the call can be captured in a HIP graph.
 * compact_every = k > 0 (joint == 0): after every k-th step the loops that stopped are taken out of the sweep's batch.  The
 *   call then SYNCHRONISES the stream there (it reads how many loops are left to size the next launches) and returns as
 *   soon as none is; not capturable.  A configuration's arithmetic does not depend on its place in the batch; the launch
 *   geometry follows the batch size, so results agree with compact_every = 0 to fp32 rounding of the sums, not bit for bit. */
typedef struct dcx_escape_opts {
    float lr, beta1, beta2, eps;       /* torch.optim.Adam: lr 5e-2 (escape.py:12), betas 0.9 / 0.999, eps 1e-8        */
    int32_t n_steps;                   /* N_WAYPOINTS (escape.py:10): the most checks a loop makes                      */
    int32_t record_freq;               /* escape.py:13; 0 or None = final configuration only                            */
    int32_t joint;
    int32_t compact_every;             /* 0 = never; k > 0 (independent loops only): see above                          */
    uint64_t wrap_mask;
} dcx_escape_opts;
size_t dcx_escape_work_bytes(const dcx_model* m, int64_t B);
int dcx_escape_adam(const dcx_model* m, float* q, int64_t B, const float* margin, const dcx_escape_opts* opt, void* work,
                    size_t work_bytes, float* history, int32_t* steps, void* stream);

/* ---- batched motion checks (added under DCX_VERSION 109) ------------------------------------------------ */
/* Is the straight joint-space motion qa[e] -> qb[e] free, and if not, which sample is the first to collide?  E edges
 * (qa, qb: [E, dof] device floats), linear interpolation, exactly one sampling rule per call:
 *   res > 0 (max_step = 0):      samples qa + (i / res)(qb - qa), i = 0 .. res - 1 (the target excluded): the point set of
 *                                Perceptron.line_predict(qa, qb, res)
 *   max_step > 0 (res = 0):      with L = |qb - qa|_2 and n = ceil(L / max_step): qa + k (max_step / L)(qb - qa) for
 *                                k = 0 .. n - 1, then qb - the point set of utils.dense_path([qa, qb], max_step).  L = 0: qb.
 * A sample collides iff score_c(q) - margin_c > 0 for some class c (margin: [C] device floats, NULL = 0).
 * first_hit [E] (int32, device, out): the smallest colliding sample index, -1 for a free edge, -2 for an edge that needs more
 *   than max_samples samples (not checked).  n_samples [E] (int32, device, out, may be NULL): the edge's sample count (the
 *   count it would need, saturated at INT32_MAX, for an edge over max_samples).
 * Samples behind an edge's first hit may be left unscored.  Three launches on the caller's stream (two small ones for the
 * sample counts and their scan, then one fused interpolate -> FK -> score-only sweep -> compare launch); no allocation,
 * no synchronisation, nothing read back: the call can be captured.
 * work: dcx_motion_work_bytes(model, E) bytes of device memory, the caller's; initialised by the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / opt / qa / qb / first_hit / work (E > 0), E < 0,
 *   both or neither of res and max_step, max_samples < 1, work_bytes below dcx_motion_work_bytes.                         */
typedef struct dcx_motion_opts {
    int32_t res;          /* > 0: the res rule;  0: the max_step rule                                                  */
    float max_step;       /* > 0: the max_step rule;  0: the res rule                                                  */
    int32_t max_samples;  /* >= 1: edges needing more samples are answered -2.  It also sizes the launch (E *
                             max_samples / 64 blocks, the surplus leaving at once): keep it close to the longest edge      */
    int32_t reserved;     /* 0                                                                                         */
} dcx_motion_opts;
size_t dcx_motion_work_bytes(const dcx_model* m, int64_t E);
int dcx_check_motions(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_opts* opt,
                      const float* margin, int32_t* first_hit, int32_t* n_samples, void* work, size_t work_bytes, void* stream);

/* ---- differentiable motion costs (added under DCX_VERSION 109) ------------------------------------------ */
/* The collision cost of the straight motion qa[e] -> qb[e] and its gradients with respect to both endpoints, E edges per call,
 * on dcx_check_motions' sample set (exactly one rule per call, see above):
 *   cost[e] = weight * sum over the edge's samples x_k of sum_c max(0, score_c(x_k) - margin_c)
 * the optimisers' collision term (reference optim.py:88-89; ScoreModel.score_hinge_grad_raw) summed over an edge: the dense-check
 * term of Weighted.step (optim.py:708-711), the per-segment con_collision_free of the SLSQP / trust-constr drivers
 * (optim.py:190-207, :350-367), on the points of utils.dense_path (utils.py:87-).
 * grad_a[e] = d cost[e] / d qa[e], grad_b[e] = d cost[e] / d qb[e] [E, dof], chained through the interpolation with the sample
 * counts held constant (as autograd through utils.dense_path holds them):
 *   res rule:      d x_k / d qb = (k / res) I
 *   max_step rule: x_k = qa + k max_step u, u = (qb - qa) / L:  d x_k / d qb = (k max_step / L)(I - u u^T),
 *                  d x_k / d qa = I - d x_k / d qb;  the target sample qb carries identity to grad_b.
 * open_end (max_step rule only; the res rule never samples qb): the target is not a sample, so the edges of a path plus its last
 *   waypoint cover utils.dense_path(p) once.  L = 0: the one sample is qb; with open_end there is none and the cost is 0.
 * An edge over max_samples: cost, grad_a and grad_b NaN; n_samples (may be NULL) holds the count it would need.
 * margin: [C] device floats, NULL = 0 (any C <= DCX_MAX_C, each class its own margin, as dcx_score_hinge_grad_mc).
 * Launches on the caller's stream: the sample counts and their scan, one fused interpolate -> FK -> score + gradient sweep
 * -> hinge -> J^T launch (C == 1; C > 1: a score pass, then the gradient sweep on the tiles that hold a sample above its
 * margin), and a per-edge reduction in sample order (no atomics: repeated calls give the same bits).  No allocation, no
 * synchronisation, nothing read back: the call can be captured.
 * work: dcx_motion_cost_work_bytes(model, E, max_samples) bytes of device memory, the caller's; initialised by the call itself
 *   (it holds per-sample values: about (dof + C + 1) * 4 bytes per possible sample).
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / opt / qa / qb / cost / grad_a / grad_b / work
 *   (E > 0), E < 0, both or neither of res and max_step, max_samples < 1, open_end not 0 / 1, reserved not 0, work_bytes below
 *   dcx_motion_cost_work_bytes.                                                                                           */
typedef struct dcx_motion_cost_opts {
    int32_t res;          /* > 0: the res rule;  0: the max_step rule                                                  */
    float max_step;       /* > 0: the max_step rule;  0: the res rule                                                  */
    int32_t max_samples;  /* >= 1: edges needing more samples answer NaN.  It sizes the launch and the workspace          */
    int32_t open_end;     /* 1: the max_step rule without the target sample;  0: with it (dcx_check_motions' set)       */
    int32_t reserved[4];  /* 0                                                                                         */
} dcx_motion_cost_opts;
size_t dcx_motion_cost_work_bytes(const dcx_model* m, int64_t E, int32_t max_samples);
int dcx_motion_cost(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_cost_opts* opt,
                    const float* margin, float weight, float* cost, float* grad_a, float* grad_b, int32_t* n_samples, void* work,
                    size_t work_bytes, void* stream);

/* ---- motions along the shortest arc of circular coordinates (added under DCX_VERSION 109) ---------------- */
/* dcx_check_motions_ex / dcx_motion_cost_ex: the two calls above with a per-coordinate wrap mask.  Bit j of wrap_mask set:
 * coordinate j is an angle on the circle and the edge runs along its shortest arc (a revolute planar arm's joints, the heading
 * of an SE(2) body, the Euler angles of an SE(3) body, a URDF `continuous` joint).  wrap_mask = 0 is the plain call, bit for
 * bit; dcx_check_motions / dcx_motion_cost forward with 0.  Everything else - the opts structs and their reserved rules, the
 * workspace sizes, the launches, no allocation / synchronisation / read-back, capturable - is as above.
 * All arithmetic fp32, each operation rounded on its own (no fused multiply-add on a masked coordinate):
 *   wrap2pi(x) = fmodf(pi + x, 2 pi), + 2 pi if that is negative, - pi; pi = 3.14159265358979323846f, 2 pi =
 *                6.28318530717958647692f (utils.wrap2pi, Python's %: the escape loop's wrap, one definition for both)
 *   delta:       d_j = wrap2pi(qb_j - qa_j) for masked j (the subtraction rounded first), qb_j - qa_j otherwise.  Masked
 *                deltas lie in [-pi, pi): a difference of exactly pi goes the negative way, as utils.anglin's
 *   res rule:    x_k,j = wrap2pi(qa_j + d_j * (k / res)) for masked j, k = 0 .. res - 1: utils.anglin(qa, qb, res,
 *                endpoint=False).  Unmasked j: the plain call's points
 *   max_step:    L = |d|_2 accumulated over j = 0 .. dof - 1 as the plain call accumulates it; n and frac = (1 / L) * max_step
 *                from L as above; x_k,j = wrap2pi(qa_j + k * (d_j * frac)) for masked j and the interior samples; the target
 *                sample is qb as given, not wrapped again; open_end as above.  L = 0 after wrapping (qb = qa + 2 pi): the one
 *                sample qb, or none with open_end and a cost of 0
 *   gradients:   wrap2pi has slope 1: the chain above with u = d / L from the wrapped delta; sample counts stay constants
 * Argument errors (DCX_ERR_INVALID, before any device work): those of the plain calls, and a wrap_mask bit at or above dof. */
int dcx_check_motions_ex(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_opts* opt,
                         const float* margin, int32_t* first_hit, int32_t* n_samples, void* work, size_t work_bytes,
                         uint64_t wrap_mask, void* stream);
int dcx_motion_cost_ex(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_cost_opts* opt,
                       const float* margin, float weight, float* cost, float* grad_a, float* grad_b, int32_t* n_samples, void* work,
                       size_t work_bytes, uint64_t wrap_mask, void* stream);

/* ---- worst-sample motion queries (added under DCX_VERSION 109) ------------------------------------------- */
/* How close does the straight motion qa[e] -> qb[e] come, where along it, and against which class?  E edges per call on exactly
 * dcx_check_motions_ex's sample set (one rule per call; res rule: samples k = 0 .. res - 1; the closed max_step rule: the
 * interior samples, then qb; wrap_mask as in the _ex calls, the points the same bits).  There is no open_end: a peak does not
 * mind a waypoint scored twice.  opt->reserved must be 0.
 *   sample value   v_k = max over c < C of (score_c(x_k) - margin_c);  margin: [C] device floats, NULL = 0.  A NaN class score
 *                  counts as -inf (dcx_check_motions never reports such a sample either); -0 counts as +0
 *   worst [E]        (float, device, out)                max_k v_k
 *   worst_idx [E]    (int32, device, out)                the smallest k that attains it
 *   worst_class [E]  (int32, device, out, may be NULL)   the smallest c that attains v_k at that k
 *   n_samples [E]    (int32, device, out, may be NULL)   as dcx_check_motions'
 * For the same (model, E, max_samples) the sweep takes the rows, slices, wave-group shares and split decision of
 * dcx_check_motions, so worst[e] > 0 exactly where that call reports a hit.  The results do not depend on the launch geometry's
 * block arrival order; repeated calls return the same bits.
 * An edge over max_samples: worst NaN, worst_idx -2, worst_class -1, its gradient rows NaN; n_samples holds the count it needs.
 * grad_a, grad_b [E, dof] (device, out; both or neither): the gradient of worst[e] with respect to qa[e] and qb[e] through the
 *   worst sample only - with g = d score_c / dq of the winning class at that sample, dcx_motion_cost's per-sample chain:
 *   res rule, t = k / res:           grad_b = t g,  grad_a = (1 - t) g
 *   max_step rule, interior sample:  grad_b = (k max_step / L)(I - u u^T) g,  grad_a = g - grad_b;  u = d / L from the wrapped
 *                                    delta where coordinates are masked; the sample count is held constant
 *   max_step rule, the target:       grad_b = g,  grad_a = 0
 * Launches on the caller's stream only: the sample counts and their scan, the reset of the per-edge keys, one fused interpolate
 * -> FK -> score-only sweep -> packed 64-bit maximum per edge, a per-edge finish; with gradients one score+gradient launch of
 * the library on the E worst samples and a chain kernel.  No synchronisation, nothing read back: the call can be captured.
 * Without gradients nothing is allocated.  The gradient launch is dcx_score_grad's, with that call's rule: a batch small enough
 * to split its supports over several blocks keeps their partial rows in the model's per-stream scratch, which is allocated
 * (hipMalloc) on the stream's first such launch outside a capture; while a stream without that scratch is being captured the
 * launch runs unsplit.  So grad_a / grad_b are the same bits on every call in the same state of the stream, but a call
 * captured on a stream that has never run a small dcx_score / dcx_score_grad / gradient call of this model may differ from the
 * eager call in the rounding of the gradient sum (worst, worst_idx, worst_class and n_samples never do).  One eager call on
 * the stream before the capture, as for dcx_score_grad, makes the two identical.
 * work: dcx_motion_worst_work_bytes(model, E) bytes of device memory, the caller's; initialised by the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): those of dcx_check_motions_ex (NULL model / opt / qa / qb / work
 *   (E > 0), E < 0, both or neither of res and max_step, max_samples < 1, a wrap_mask bit at or above dof), NULL worst or
 *   worst_idx (E > 0), exactly one of grad_a / grad_b, reserved not 0, work_bytes below dcx_motion_worst_work_bytes.
 *   max_samples above 2^24 - 1 is DCX_ERR_UNSUPPORTED.                                                                    */
size_t dcx_motion_worst_work_bytes(const dcx_model* m, int64_t E);
int dcx_motion_worst(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_opts* opt,
                     const float* margin, float* worst, int32_t* worst_idx, int32_t* worst_class, int32_t* n_samples,
                     float* grad_a, float* grad_b, void* work, size_t work_bytes, uint64_t wrap_mask, void* stream);

/* ---- hybrid motion checks (added under DCX_VERSION 109) --------------------------------------------------- */
/* A two-threshold motion check: the proxy's verdict where its score is clearly above hi or clearly at or below lo, and a compact,
 * ordered list of exactly those samples that still need a ground-truth checker (the reference's HybridForwardKinematicsDiffCo,
 * collision_checkers.py:511-548, for motions).  E edges per call on exactly dcx_check_motions_ex's sample set, bit for bit (one
 * rule per call: the res rule or the closed max_step rule; wrap_mask as there).  opt->reserved must be 0.
 *   lo, hi         [C] device floats, NULL = 0 for that side
 *   sample code    from the class scores s_c of sample k:  hit_k = some c has s_c - hi_c > 0 (dcx_check_motions' comparison with
 *                  margin = hi);  clear_k = every c has s_c - lo_c <= 0;  code 1 if hit_k, else 0 if clear_k, else 2.  A NaN
 *                  class score is neither a hit nor clear: the sample is uncertain.  lo_c > hi_c is the caller's error: hit wins
 *   verdict [E]      (int32, device, out)                1 if a sample has code 1, else 2 if one has code 2, else 0;
 *                                                        -2 for an edge over max_samples (not checked)
 *   first_hit [E]    (int32, device, out, may be NULL)   the smallest k with code 1, -1 none, -2 over max_samples
 *   n_samples [E]    (int32, device, out, may be NULL)   as dcx_check_motions'
 *   n_uncertain [E]  (int32, device, out, may be NULL)   the code-2 samples of an edge with verdict 2; 0 for every other edge
 *                                                        (an edge with a sure hit is decided: its band samples do not count)
 *   unc_total [1]    (int64, device, out)                the sum of n_uncertain; may exceed unc_cap
 *   unc_edge, unc_sample [unc_cap] (int32, device, out)  the code-2 samples of the verdict-2 edges, ordered by (edge, sample)
 *                                                        ascending: entry j at index j for j < unc_cap, nothing written at or
 *                                                        beyond unc_cap
 *   unc_q [unc_cap, dof] (float, device, out, may be NULL) the listed samples' configurations as the sweep evaluated them
 * An edge over max_samples: verdict -2, first_hit -2, n_uncertain 0, nothing listed; n_samples holds the count it needs.
 * For the same (model, E, max_samples) the sweep takes the rows, slices, wave-group shares and split decision of
 * dcx_check_motions, so first_hit equals dcx_check_motions_ex(margin = hi)'s with no tolerance, and verdict == 0 exactly where
 * dcx_motion_worst(margin = lo) reports worst <= 0 (NaN scores aside).
 * Launches on the caller's stream only: the sample counts and their scan, one fused interpolate -> FK -> score-only sweep ->
 * one code byte per sample, then a per-edge pass over the codes in sample order, a scan of the per-edge counts and the scatter
 * of the list.  No allocation, no synchronisation, nothing read back: the call can be captured.  No atomics decide the order
 * of anything; repeated calls return the same bits.
 * work: dcx_motion_band_work_bytes(model, E, max_samples) bytes of device memory, the caller's; initialised by the call itself
 *   (dcx_check_motions' workspace, then one byte per possible sample and 12 bytes per edge).
 * Argument errors (DCX_ERR_INVALID, before any device work): those of dcx_check_motions_ex (NULL model / opt / qa / qb / work
 *   (E > 0), E < 0, both or neither of res and max_step, max_samples < 1, a wrap_mask bit at or above dof), out NULL, verdict or
 *   unc_total NULL (E > 0), unc_cap < 0, unc_edge or unc_sample NULL with unc_cap > 0, reserved not 0 (opt's or out's),
 *   work_bytes below dcx_motion_band_work_bytes.  E above 2^31 - 1, E * max_samples too large for one launch and a feature
 *   width without a kernel are DCX_ERR_UNSUPPORTED.  E = 0 launches nothing and writes nothing.                             */
typedef struct dcx_motion_band_out {
    int32_t* verdict;      /* [E] out: 0 free, 1 collides, 2 uncertain, -2 over max_samples (not checked)          */
    int32_t* first_hit;    /* [E] out, may be NULL: smallest sample above hi, -1 none, -2 over max_samples          */
    int32_t* n_samples;    /* [E] out, may be NULL: as dcx_check_motions'                                            */
    int32_t* n_uncertain;  /* [E] out, may be NULL: band samples of an edge with verdict 2; 0 for every other edge   */
    int64_t* unc_total;    /* [1] out: sum of n_uncertain; may exceed unc_cap                                        */
    int32_t* unc_edge;     /* [unc_cap] out                                                                          */
    int32_t* unc_sample;   /* [unc_cap] out                                                                          */
    float*   unc_q;        /* [unc_cap, dof] out, may be NULL: the listed samples' configurations                    */
    int64_t  unc_cap;      /* >= 0                                                                                   */
    int64_t  reserved[2];  /* 0                                                                                      */
} dcx_motion_band_out;
size_t dcx_motion_band_work_bytes(const dcx_model* m, int64_t E, int32_t max_samples);
int dcx_motion_band(const dcx_model* m, const float* qa, const float* qb, int64_t E, const dcx_motion_opts* opt,
                    const float* lo, const float* hi, const dcx_motion_band_out* out, void* work, size_t work_bytes,
                    uint64_t wrap_mask, void* stream);

/* ---- k-nearest neighbours (added under DCX_VERSION 109) -------------------------------------------------- */
/* The k nearest of N points for each of Q queries under the motion calls' metric: the producer of their (qa, qb).  No model.
 * Distance: the squared length of the edge query -> point exactly as dcx_check_motions_ex(qa = query, qb = point, wrap_mask)
 *   accumulates it: d_j = point_j - query_j (rounded), along the shortest arc (wrap2pi of it) where bit j of wrap_mask is set;
 *   l2 = l2 + d_j * d_j for j = 0 .. dof - 1 from +0.0f, every operation fp32 and rounded on its own (no fused multiply-add).
 *   dist2 holds the very bits whose square root is the motion call's edge length L.  Under a wrap mask the value depends on the
 *   direction: wrap2pi(x) and -wrap2pi(-x) may differ in their last bits, so dist2(query -> point) need not equal
 *   dist2(point -> query) bit for bit.
 * Order: neighbours are totally ordered by (dist2, point index) ascending, the lower index winning a tie.  dist2 is never negative
 *   or -0, so its bit pattern orders like its value: the key is bits(dist2) << 32 | index.
 * Row i of idx / dist2 holds the first k of that order over the admissible points.  Not admissible: a point whose dist2 is NaN,
 *   one whose dist2 is above max_dist2, and point self_offset + i (self_offset >= 0).  Unfilled slots: idx -1, dist2 +inf.
 * The result is a function of the inputs alone: it does not depend on how the launch is split, and nothing is atomic.
 * Launches on the caller's stream only (a search over (query tiles) x (point splits), then a merge of the splits' lists where
 * there are several).  No allocation, no synchronisation, nothing read back: the call can be captured.
 * work: dcx_knn_work_bytes(Q, N, dof, k) bytes of device memory, the caller's; initialised by the call itself.
 * Q == 0 returns 0 and touches nothing; N == 0 fills -1 / +inf.
 * Argument errors (DCX_ERR_INVALID, before any device work): opt NULL; queries / idx / dist2 / work NULL (Q > 0), points NULL
 *   (Q > 0 and N > 0); Q < 0 or N < 0; dof outside 1 .. 64; k outside 1 .. DCX_KNN_MAX_K; a wrap_mask bit at or above dof; a NaN
 *   or negative max_dist2; self_offset < -1; a reserved field not 0; work_bytes below dcx_knn_work_bytes.  N above 2^31 - 1 and
 *   a grid beyond one launch are DCX_ERR_UNSUPPORTED.  dcx_knn_work_bytes is 0 for arguments dcx_knn refuses.               */
#define DCX_KNN_MAX_K 64
typedef struct dcx_knn_opts {
    int32_t  k;            /* 1 .. DCX_KNN_MAX_K                                                        */
    int32_t  reserved0;    /* 0                                                                          */
    uint64_t wrap_mask;    /* bit j: coordinate j is an angle, measured along the shortest arc           */
    float    max_dist2;    /* keep only neighbours with dist2 <= max_dist2; +inf: no radius              */
    int32_t  reserved1;    /* 0                                                                          */
    int64_t  self_offset;  /* >= 0: query i IS point self_offset + i and is not its own neighbour; -1: none */
    int64_t  reserved[2];  /* 0                                                                          */
} dcx_knn_opts;
size_t dcx_knn_work_bytes(int64_t Q, int64_t N, int32_t dof, int32_t k);
int dcx_knn(int device, const float* queries, int64_t Q, const float* points, int64_t N, int32_t dof, const dcx_knn_opts* opt,
            int32_t* idx, float* dist2, void* work, size_t work_bytes, void* stream);

/* ---- dense-check Adam trajectory loop (added under DCX_VERSION 109) --------------------------------------- */
/* dcx_traj_adam_run charges the collision hinge at the waypoints only; here it is charged along the segments: the dense-check
 * form of Weighted.step (optim.py:706-752 with dense_check=True).  R independent paths p = path[r] [W, dof]; one iteration:
 *   sample set   the points of utils.dense_path(p, max_step): for w < W - 1 the OPEN max_step edge p[w] -> p[w+1]
 *                (dcx_motion_cost_ex's samples with open_end = 1), then the single sample p[W-1] (the closed zero-length edge
 *                p[W-1] -> p[W-1]).  wrap_mask != 0: every edge along the shortest arc, exactly as in dcx_motion_cost_ex
 *   collision    coll_sum = sum over the N_r samples x_k and the classes c of max(0, score_c(x_k) - margin_c)
 *                normalize = 0: collision = coll_sum                    (ScoreModel.path_cost, the scipy drivers' sum)
 *                normalize = 1: collision = coll_sum * W / (N_r * C)    (Weighted's .mean() * len(p))
 *                gradients through the interpolation with the sample counts, and so N_r, held constant (dcx_motion_cost)
 *   the rest     as dcx_traj_adam_step: path length in control-point space, max-move, joint limits, Adam with bias correction,
 *                stats[r, 0..6] (stats[r, 4] = collision as defined above), lowest-loss / best-valid bookkeeping, steps, the
 *                valid_tol / grad_tol stop
 *   move [W]     bytes, device, may be NULL: a waypoint whose byte is 0 gets a zero gradient (Weighted's mask, shared by the R
 *                paths).  NULL: the two endpoints are fixed, dcx_traj_adam_step's rule
 *   rewrap_mask  after the Adam update coordinate j with bit j set becomes wrap2pi(q_j) (the escape loop's function, see
 *                dcx_motion_cost_ex) - robot.wrap after opt.step().  Independent of the SAMPLING wrap_mask: the reference wraps
 *                after the step but samples linearly
 *   stop_tol > 0 a path whose constraint value of THIS iteration (stats[r, 2]) is <= stop_tol takes this step and is then
 *                frozen (done[r] = 1): Weighted's `if constraint_loss <= 0.5: break` after opt.step().  0: no such stop
 *   history      may be NULL: [n_iters, R, W, dof], the path after each step of this call; a frozen path's row repeats
 *   n_checks [R] int64, device, in/out: samples scored so far (+= N_r per step taken)
 *   an edge needing more than max_samples samples (dcx_motion_cost_ex answers NaN; so does a NaN cost): the path takes NO step
 *                and is frozen - done[r] = 1, stats[r, 7] = -2, and path, moments, bookkeeping, steps, n_checks and
 *                stats[r, 0..6] are untouched (its history row is the unchanged path)
 * The per-edge arrays of dcx_traj_dense_io hold dcx_motion_cost_ex's outputs (weight = 1) in the layout e = r * W + w: slot
 * w < W - 1 is the open edge leaving waypoint w, slot W - 1 the closed zero-length edge on the last waypoint (its grad_a 0, its
 * grad_b the hinge gradient at p[W-1], its n_samples 1).  The collision gradient of waypoint w is grad_a[e(r, w)] +
 * grad_b[e(r, w-1)] (no left neighbour at w = 0; at w = W - 1 the closed edge's grad_b as well), scaled by w_collision and,
 * under normalize, by W / (N_r * C).  N_r and coll_sum are summed in waypoint order: repeated calls return the same bits.
 *
 * dcx_traj_dense_step: the step half alone, ONE launch on per-edge arrays that already hold this iteration's motion costs;
 *   st->col_score / st->col_grad are not read and may be NULL; io->history, if given, is THIS step's row [R, W, dof]; C is
 *   the class count of the normalisation.
 * dcx_traj_dense_run: n_iters iterations on the caller's stream, starting at 1-based step first_step; per iteration
 *   1. an edge-list launch (the shifted path qb[e] = p[min(w + 1, W - 1)] beside qa = path itself, and the R last waypoints)
 *   2. dcx_motion_cost_ex's launches twice: the R * W open slots (slot W - 1 is zero-length: no sample, cost 0), then the R
 *      closed edges, whose results a small launch copies into slot W - 1
 *   3. the dense step
 *   The per-edge results go into the io arrays, or into the workspace where the caller leaves all four NULL.  margin: [C]
 *   DEVICE floats as in the motion calls; NULL = opt->safety_margin for every class (kept in the workspace).  No allocation,
 *   no synchronisation, nothing read back: the call can be captured.  work: dcx_traj_dense_work_bytes(model, R, W,
 *   max_samples) bytes of device memory, the caller's; initialised by the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / st / opt / dopt / io / n_checks / work / a state
 *   pointer (R > 0), the per-edge arrays partly NULL (dcx_traj_dense_step: any of them NULL), n_iters < 0, first_step or step
 *   < 1, max_step <= 0, max_samples < 1, normalize not 0 / 1, stop_tol < 0, a wrap_mask or rewrap_mask bit at or above dof,
 *   reserved not 0, work_bytes below dcx_traj_dense_work_bytes.  W outside 2 .. 1024: DCX_ERR_UNSUPPORTED.            */
typedef struct dcx_traj_dense_opts {
    float max_step;        /* > 0: the sampling stride (Weighted: max_speed)                                            */
    int32_t max_samples;   /* >= 1: a path with an edge needing more is frozen (-2).  It sizes the launches and the work  */
    uint64_t wrap_mask;    /* sampling: bit j = coordinate j runs along its shortest arc                                  */
    uint64_t rewrap_mask;  /* after the update: bit j = coordinate j is wrapped to [-pi, pi)                              */
    int32_t normalize;     /* 0: collision = coll_sum;  1: coll_sum * W / (N_r * C)                                       */
    float stop_tol;        /* > 0: freeze after the step whose constraint is <= stop_tol;  0: off                         */
    int32_t reserved[4];   /* 0                                                                                         */
} dcx_traj_dense_opts;
typedef struct dcx_traj_dense_io {
    const uint8_t* move;   /* [W] or NULL                                                                                */
    float* history;        /* run: [n_iters, R, W, dof];  step: [R, W, dof];  or NULL                                    */
    int64_t* n_checks;     /* [R] in/out                                                                                 */
    float* edge_cost;      /* [R * W]                                                                                    */
    float* grad_a;         /* [R * W, dof]                                                                               */
    float* grad_b;         /* [R * W, dof]                                                                               */
    int32_t* n_samples;    /* [R * W]                                                                                    */
} dcx_traj_dense_io;
int dcx_traj_dense_step(int device, const dcx_fk_desc* fk, const dcx_traj_state* st, const dcx_traj_opts* opt,
                        const dcx_traj_dense_opts* dopt, const dcx_traj_dense_io* io, int32_t C, int32_t step, void* stream);
size_t dcx_traj_dense_work_bytes(const dcx_model* m, int32_t R, int32_t W, int32_t max_samples);
int dcx_traj_dense_run(const dcx_model* m, const dcx_traj_state* st, const dcx_traj_opts* opt, const dcx_traj_dense_opts* dopt,
                       const dcx_traj_dense_io* io, const float* margin, int32_t first_step, int32_t n_iters, void* work,
                       size_t work_bytes, void* stream);

/* ---- batched RRT-Connect (added under DCX_VERSION 109) ---------------------------------------------------- */
/* R independent planning problems grown in lockstep, P = opts->slots extensions per problem and round: the tree planner over
 * dcx_knn's metric and dcx_check_motions_ex's verdicts (the reference's scripts/motion_planner.py hands OMPL's RRTConnect a
 * DiffCo validity checker; misc/rrt_star.py grows a tree over line_collision).  All tree logic runs on the device, the edge
 * checks are dcx_check_motions_ex's own launches, and nothing is read back between rounds.
 * State (dcx_rrt_state; caller-owned device memory, R problems, cap = opts->cap):
 *   nodes [R, 2, cap, dof] float    tree 0 is rooted at the start (node 0, parent -1), tree 1 at the goal
 *   parent [R, 2, cap] int32        count [R, 2] int32: the trees' sizes (>= 1)
 *   status [R] int32                0 running, 1 solved, 2 a tree is full, 3 an endpoint collides (set by the caller when it
 *                                   initialises the state, never by the kernels)
 *   link [R, 2] int32               of a solved problem: (index in tree 0, index in tree 1) of the two nodes the free joining
 *                                   motion connects
 *   solved_round [R] int32          of a solved problem: the round g that solved it
 * Round g = round0 + t, t = 0 .. T - 1: tree a = g & 1 extends, tree b = 1 - a connects.  Both phases see each tree as it stood
 * at the start of the round.  A problem's status is read at the start of the round and written only at its end; a problem that
 * is not running (status != 0) is left as it is.  Solved wins over full.
 * Phase 1, extend - slot p < P of a running problem r:
 *   1. target s = samples[t, r, p, :]
 *   2. near = the nearest node of tree a under dcx_knn's contract (query = s, points = the tree's nodes, k = 1): the same dist2
 *      bits (d = node - s, wrapped on masked coordinates, summed from +0 in coordinate order, every operation rounded alone),
 *      the same key order bits(dist2) << 32 | index; a NaN distance is not admitted.  No admissible node: the slot is idle
 *   3. steer, every operation fp32 and rounded alone: d_j = the motion calls' delta of the edge near -> s (wrap2pi of the
 *      rounded difference on masked j), l2 = l2 + d_j * d_j from +0 in coordinate order, L = sqrtf(l2) (correctly rounded) as
 *      dcx_check_motions_ex forms an edge's length.  !(L > 0): the slot is idle.  L <= range: qb = s as given.  Otherwise
 *      f = range / L (one correctly rounded division) and qb_j = near_j + d_j * f, then wrap2pi on masked j
 *   4. the edge near -> qb is checked by dcx_check_motions_ex (the closed max_step rule, opts->max_samples, margin, wrap_mask):
 *      first_hit == -1 accepts the slot, anything else (-2 included) rejects it
 *   5. commit: the accepted slots append qb to tree a in ascending slot order with parent = near while count < cap; a slot that
 *      does not fit is dropped and marks the problem full
 * Phase 2, connect - each slot whose node x was appended in phase 1:
 *   1. nb = the nearest node of tree b under the same contract, query = x
 *   2. the edge nb -> x is checked (the closed max_step rule; not capped at range)
 *   3. first_hit == -1: the slot joins.  The joining slot with the lowest p sets status = 1, link and solved_round = g
 *   4. first_hit = h >= 2: sample h - 1 of that edge - the last free one - is appended to tree b with parent = nb: bit for bit
 *      the point dcx_check_motions_ex scored (x_k of the max_step rule above with the call's own frac), in the same slot order
 *      and under the same cap rule as phase 1.  Every slot of a round appends what it has, also beside a joining slot
 *   5. h in {0, 1, -2}: nothing is appended
 * Fixed batch: every phase of every round submits exactly R * P edges in (r, p) order.  Idle, dropped and non-running slots
 *   submit the edge nodes[r, 0, 0] -> nodes[r, 0, 0] (one sample, its verdict ignored), so the geometry of the motion sweep never
 *   depends on the state: the call can be captured, and a referee that submits the same batch to dcx_check_motions_ex gets the
 *   same verdicts.
 * dcx_rrt_connect_run enqueues T rounds on the caller's stream: per round and phase one nearest (+ steer) launch, the launches
 *   of dcx_check_motions_ex, one commit launch.  No allocation, no synchronisation, no atomic decides any order, nothing read
 *   back; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.
 *   samples [T, R, P, dof] device floats;  margin [C] device floats, NULL = 0.
 * work: dcx_rrt_work_bytes(model, R, slots) bytes of device memory, the caller's (dcx_check_motions' workspace for R * P edges,
 *   then the per-slot scratch: the edge batch, its verdicts and append indices); initialised by the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / opts; NULL state, state pointer, samples (T > 0) or
 *   work with R > 0; R < 0 or T < 0; round0 < 0 or round0 + T above 2^31 - 1; range or max_step <= 0 or NaN; max_samples < 1;
 *   slots outside 1 .. DCX_RRT_MAX_SLOTS; cap outside 1 .. DCX_RRT_MAX_CAP; a wrap_mask bit at or above dof; a reserved field
 *   not 0; work_bytes below dcx_rrt_work_bytes.  R * slots above 2^31 - 1, R * slots * max_samples too large for one launch,
 *   dof above DCX_MAX_DOF and a feature width without a motion kernel are DCX_ERR_UNSUPPORTED.  R = 0 or T = 0 launches nothing.
 *   dcx_rrt_work_bytes is 0 for arguments the call refuses.                                                                  */
#define DCX_RRT_MAX_SLOTS 16
#define DCX_RRT_MAX_CAP 1048576
typedef struct dcx_rrt_state {
    float*   nodes;         /* [R, 2, cap, dof]                                                             */
    int32_t* parent;        /* [R, 2, cap]                                                                  */
    int32_t* count;         /* [R, 2]                                                                       */
    int32_t* status;        /* [R]: 0 running, 1 solved, 2 full, 3 an endpoint collides                     */
    int32_t* link;          /* [R, 2]                                                                       */
    int32_t* solved_round;  /* [R]                                                                          */
} dcx_rrt_state;
typedef struct dcx_rrt_opts {
    float    range;        /* > 0: the longest extension of phase 1                                         */
    float    max_step;     /* > 0: the sampling stride of every edge check                                  */
    int32_t  max_samples;  /* >= 1: an edge needing more samples is rejected; it sizes the sweep launches   */
    int32_t  slots;        /* P, 1 .. DCX_RRT_MAX_SLOTS                                                     */
    int32_t  cap;          /* nodes per tree, 1 .. DCX_RRT_MAX_CAP                                          */
    int32_t  reserved0;    /* 0                                                                             */
    uint64_t wrap_mask;    /* bit j: coordinate j is an angle, measured and walked along the shortest arc   */
    int64_t  reserved[2];  /* 0                                                                             */
} dcx_rrt_opts;
size_t dcx_rrt_work_bytes(const dcx_model* m, int64_t R, int32_t slots);
int dcx_rrt_connect_run(const dcx_model* m, const dcx_rrt_state* state, int64_t R, const float* samples, int32_t T, int64_t round0,
                        const dcx_rrt_opts* opts, const float* margin, void* work, size_t work_bytes, void* stream);

/* ---- batched RRT* (added under DCX_VERSION 109) ----------------------------------------------------------- */
/* R independent planning problems, one tree each, grown in lockstep with P = opts->slots extensions per problem and round: the
 * asymptotically optimal tree planner over dcx_knn's metric and dcx_check_motions_ex's verdicts (the reference's
 * misc/rrt_star.py grows one tree, links each new node and rewires every node within a fixed radius whose cost-to-come improves
 * over a free line_collision motion).  Only path length under the motion calls' metric is optimised.  All tree logic runs on the
 * device, the edge checks are dcx_check_motions_ex's own launches, and nothing is read back between rounds.
 * State (dcx_rrtstar_state; caller-owned device memory, R problems, cap = opts->cap):
 *   nodes [R, cap, dof] float       node 0 is the start
 *   parent [R, cap] int32           the root's is -1
 *   elen [R, cap] float             the length of the edge parent -> node; the root's is 0
 *   cost [R, cap] float             the cost-to-come: cost[i] = cost[parent[i]] + elen[i] (one rounded fp32 sum); the root's is +0
 *   count [R] int32                 the nodes in the tree (>= 1)
 *   status [R] int32                0 running, 1 the direct motion start -> goal is free (set by the caller when it initialises
 *                                   the state: node 1 is then the goal with parent 0, goal_node = 1, and that is the optimum),
 *                                   2 full, 3 an endpoint collides (set by the caller, never by the kernels)
 *   goal_node [R] int32             -1 until a node with the goal's bits is in the tree, then that node's index (the first one)
 *   first_round [R] int32           the round that first reached the goal, else -1
 * A problem's status is read at the start of the round and written only at its end; a problem that is not running (status != 0)
 * is left as it is.  A running problem keeps running after it has found the goal: the planner is anytime.
 * Round g = round0 + t, t = 0 .. T - 1, for a running problem r.  Every phase sees nodes, parent, cost and count as they stood
 * at the start of the round (the snapshot).  Every arithmetic step is fp32 and rounded alone.  K = opts->near.
 *   1. extend - slot p < P: dcx_rrt_connect_run's phase 1, steps 1 - 4, on the one tree: target s = samples[t, r, p, :], near =
 *      the nearest node under dcx_knn's contract (query = s, k = 1), the steering to opts->range giving x, the edge near -> x
 *      checked by dcx_check_motions_ex.  first_hit == -1 makes slot p a candidate with L0 = L(near -> x), the motion call's
 *      own length bits: d_j = the motion calls' delta of the edge near -> x, l2 = l2 + d_j * d_j from +0 in coordinate order,
 *      L = sqrtf(l2), correctly rounded.  Anything else (-2 included) leaves the slot idle for the rest of the round
 *   2. near set (K > 0) - each candidate: the first K of dcx_knn's order for query = x over the snapshot's nodes with
 *      max_dist2 = radius * radius (one rounded product): dist2_j and u_j, j < K; unfilled places are -1
 *   3. choose parent - for each u_j: Lj = L(u_j -> x) formed as in 1 for that directed edge, cj = cost[u_j] + Lj.  The incumbent
 *      is c0 = cost[near] + L0.  Place (r, p, j) submits the edge u_j -> x only where (bits(cj), u_j) < (bits(c0), near), in
 *      lexicographic order of the two unsigned numbers; every other place is idle.  The parent of x is the submitted u_j with
 *      first_hit == -1 and the least (bits(cj), u_j), with elen = Lj and cost = cj; without one it is near, with L0 and c0
 *   4. append - the candidates are appended in ascending slot order while count < cap, with parent, elen and cost from 3; a
 *      slot that does not fit is dropped and marks the problem full (status 2 at the end of the round).  With goal_node[r] == -1,
 *      the appended node of the lowest slot whose dof words equal goals[r, :] bit for bit sets goal_node to its index and
 *      first_round = g (the steering hands a sample within range through as given, so a goal-biased sampler puts the goal's own
 *      bits into the tree).  Every other copy of the goal, of this round or a later one, is an ordinary node
 *   5. rewire (K > 0) - for each appended x and each v = u_j >= 0 with v != parent(x): L' = sqrtf(dist2_j), correctly rounded:
 *      the length of the directed edge x -> v, the bits dcx_knn documents;  c' = cost[x] + L'.  Place (r, p, j) submits the edge
 *      x -> v only where c' < cost[v] on the snapshot's cost[v]; every other place is idle.  Of the submitted places with
 *      first_hit == -1 for one v across the slots, the least (bits(c'), p) wins: parent[v] = x's index, elen[v] = L'.  The
 *      selection is a compare-all in LDS, one block per problem
 *   6. refresh - cost[i] = cost[parent[i]] + elen[i] for every node from the root's +0: the unique fixed point for the new
 *      (parent, elen).  One block per problem repeats passes over its nodes until a pass changes nothing; skipped where the
 *      round rewired nothing.  The parent graph stays a tree and no node's cost ever rises (DESIGN.md 3.4o has the argument)
 * Fixed batch: the extend phase of every round submits exactly R * P edges in (r, p) order, the choose and the rewire phase
 *   R * P * K edges each in (r, p, j) order.  Idle places submit the edge nodes[r, 0] -> nodes[r, 0] (one sample, its verdict
 *   ignored), so the geometry of the motion sweeps never depends on the state: the call can be captured, and a referee that
 *   submits the same batches to dcx_check_motions_ex gets the same verdicts.  K = 0 runs the extend, append and refresh phases
 *   only: plain RRT with costs, on the same nodes as any K for equal samples - the set of nodes does not depend on the parents.
 * dcx_rrtstar_run enqueues T rounds on the caller's stream.  No allocation, no synchronisation, no atomic decides any order,
 *   nothing read back; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.
 *   goals [R, dof], samples [T, R, P, dof] device floats;  margin [C] device floats, NULL = 0.
 * DCX_RRTSTAR_MAX_CAP: the refresh is ONE block of 1024 threads per problem that sweeps parent, elen and cost of the whole tree
 *   once per pass, as many passes as the deepest rewired chain is long.  At 65536 nodes a pass is 64 nodes per thread over 768 KiB
 *   of state, which an XCD's L2 still holds beside the other problems' trees; a larger tree would turn every pass of that single
 *   block into a stream from HBM.  (The near search, a wave per slot, reads 1024 rows per lane at that size.)
 * work: dcx_rrtstar_work_bytes(model, R, slots, near) bytes of device memory, the caller's (dcx_check_motions' workspace for
 *   R * P * max(K, 1) edges, then the edge batches, their verdicts, the near lists and the candidates' costs); initialised by
 *   the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / opts; NULL state, state pointer, goals, samples (T > 0)
 *   or work with R > 0; R < 0 or T < 0; round0 < 0 or round0 + T above 2^31 - 1; range or max_step <= 0 or NaN; radius negative
 *   or NaN; max_samples < 1; slots outside 1 .. DCX_RRT_MAX_SLOTS; near outside 0 .. DCX_RRTSTAR_MAX_NEAR; cap outside
 *   1 .. DCX_RRTSTAR_MAX_CAP; a wrap_mask bit at or above dof; a reserved field not 0; work_bytes below dcx_rrtstar_work_bytes.
 *   R * slots * max(near, 1) above 2^31 - 1, R * slots * max(near, 1) * max_samples too large for one launch, dof above
 *   DCX_MAX_DOF and a feature width without a motion kernel are DCX_ERR_UNSUPPORTED.  R = 0 or T = 0 launches nothing.
 *   dcx_rrtstar_work_bytes is 0 for arguments the call refuses.                                                              */
#define DCX_RRTSTAR_MAX_NEAR 16
#define DCX_RRTSTAR_MAX_CAP 65536
typedef struct dcx_rrtstar_state {
    float*   nodes;         /* [R, cap, dof]                                                                */
    int32_t* parent;        /* [R, cap]                                                                     */
    float*   elen;          /* [R, cap]                                                                     */
    float*   cost;          /* [R, cap]                                                                     */
    int32_t* count;         /* [R]                                                                          */
    int32_t* status;        /* [R]: 0 running, 1 the direct motion is free, 2 full, 3 an endpoint collides  */
    int32_t* goal_node;     /* [R]                                                                          */
    int32_t* first_round;   /* [R]                                                                          */
} dcx_rrtstar_state;
typedef struct dcx_rrtstar_opts {
    float    range;        /* > 0: the longest extension                                                    */
    float    max_step;     /* > 0: the sampling stride of every edge check                                  */
    float    radius;       /* >= 0: the near set's radius                                                   */
    int32_t  max_samples;  /* >= 1: an edge needing more samples is rejected; it sizes the sweep launches   */
    int32_t  slots;        /* P, 1 .. DCX_RRT_MAX_SLOTS                                                     */
    int32_t  near;         /* K, 0 .. DCX_RRTSTAR_MAX_NEAR; 0: no choose-parent, no rewiring                */
    int32_t  cap;          /* nodes per tree, 1 .. DCX_RRTSTAR_MAX_CAP                                      */
    int32_t  reserved0;    /* 0                                                                             */
    uint64_t wrap_mask;    /* bit j: coordinate j is an angle, measured and walked along the shortest arc   */
    int64_t  reserved[2];  /* 0                                                                             */
} dcx_rrtstar_opts;
size_t dcx_rrtstar_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t near);
int dcx_rrtstar_run(const dcx_model* m, const dcx_rrtstar_state* state, int64_t R, const float* goals, const float* samples, int32_t T,
                    int64_t round0, const dcx_rrtstar_opts* opts, const float* margin, void* work, size_t work_bytes, void* stream);
/* The paths to the goal nodes of a dcx_rrtstar_state as rows of path [R, W, dof], one launch on `device`, without a model, with
 * dcx_rrt_extract_paths' conventions: a wave per problem walks parent from goal_node[r], at most count[r] steps, and writes the
 * n waypoints root first.  n <= W sets count_out[r] = n; n > W leaves the row untouched and sets count_out[r] = -n, so W = 0
 * (path may then be NULL) is the size query.  goal_node[r] == -1: count_out[r] = 0.  A chain that leaves 0 .. count[r] - 1 or
 * does not reach parent -1 within count[r] steps gives count_out[r] = 0, and nothing is read out of bounds.
 * Argument errors (DCX_ERR_INVALID): R < 0; cap outside 1 .. DCX_RRTSTAR_MAX_CAP; dof < 1; W < 0; with R > 0 a NULL state,
 *   nodes, parent, count, goal_node or count_out, or a NULL path with W > 0.  R above 2^31 - 1 is DCX_ERR_UNSUPPORTED.  R = 0
 *   launches nothing.                                                                                                        */
int dcx_rrtstar_extract_paths(int device, const dcx_rrtstar_state* state, int64_t R, int32_t cap, int32_t dof,
                              float* path, int32_t W, int32_t* count_out, void* stream);

/* ---- batched RRT*: samples drawn on the device (added under DCX_VERSION 109) ------------------------------ */
/* The samples of a round drawn where the trees live, from each problem's state at the start of that round: uniform in the joint
 * limits with a goal bias until the problem has a goal node, and from then on (mode informed) inside the set that can still
 * shorten its path, { x : d(start, x) + d(x, goal) <= c_best } (Gammell, Srinivasa, Barfoot: Informed RRT*, IROS 2014).  One
 * thread per slot (r, p); no scratch, no atomics, nothing read back.
 * Random numbers: Philox4x32-10.  The key is (seed's low word, seed's high word); the counter is (g, r * 16 + p, t, b): round,
 *   slot, try and block.  A uniform is (word >> 8) * 2^-24 in [0, 1); where a logarithm follows it is ((word >> 8) + 1) * 2^-24.
 *   block 0, try 0:        word 0 = u_bias decides the goal bias, word 1 = u_mix decides the uniform mix
 *   blocks 1 .. 8, try 0:  the uniform-in-limits coordinates: u_j is word j % 4 of block 1 + j / 4
 *   blocks 9 .. 17, try t: the informed draw of try t.  Word 0 of block 9 is the radial uniform u_rad.  Blocks 10 .. 17 hold one
 *                          Box-Muller pair per two coordinates: words (0, 1) of block 10 + j / 4 serve coordinates 4 b and 4 b + 1,
 *                          words (2, 3) coordinates 4 b + 2 and 4 b + 3; with (w, w') the pair, rad = sqrt(-2 ln u(w)) (the
 *                          logarithm's uniform) and (sn, cs) = sincospi(2 u(w')), the even coordinate is rad * cs, the odd rad * sn
 *   A draw depends on (seed, g, r, p) and the snapshot alone: not on T, on the chunking of the rounds into calls, or on launch
 *   geometry.
 * Slot (r, p) of a running problem (status[r] == 0) in round g, in this order; lo_j = limits[j, 0], hi_j = limits[j, 1]:
 *   1. goal     - with goal_node[r] == -1 and u_bias < goal_bias the sample is goals[r, :], bit for bit.  The bias is off once the
 *                 problem has a goal node: the goal is then reached more cheaply by rewiring, and a copy would be an ordinary node
 *   2. uniform  - otherwise, with goal_node[r] == -1, or mode == DCX_RRTSTAR_SAMPLE_UNIFORM, or u_mix < uniform_mix:
 *                 x_j = lo_j + span_j * u_j with span_j = hi_j - lo_j: one rounded fp32 product and one rounded fp32 sum (never
 *                 contracted), so a referee reproduces the bits
 *   3. informed - otherwise c = cost[r, goal_node[r]] of the snapshot.  a = the motion calls' wrapped delta start -> goal with
 *                 start = nodes[r, 0]; c_min = |a| (the motion calls' length of that edge), a^ = a / c_min, centre = start + a / 2;
 *                 r1 = c / 2, r2 = sqrt(max(c^2 - c_min^2, 0)) / 2, the difference formed as (c - c_min) (c + c_min), which keeps
 *                 its digits where c is close to c_min.  Try t = 0 .. tries - 1: z = the dof Gaussians of try t, u = z / |z| *
 *                 u_rad^(1 / dof): a uniform point of the unit ball;  y = (r1 u_0, r2 u_1, .., r2 u_{dof-1});  x = centre + H y,
 *                 H the Householder reflection that takes e_0 to -+a^: v = a^ + sign(a^_0) e_0 (sign(0) = +1),
 *                 H y = y - 2 v (v.y) / (v.v).  O(dof) per try, no rotation matrix; v.v = 2 (1 + |a^_0|) >= 2, so it is stable
 *                 everywhere, and the sign does not matter because the ball is symmetric.  Coordinates of the wrap mask are brought
 *                 into [-pi, pi) as the steering step's.  The first try with lo_j <= x_j < hi_j for every j is the sample; without
 *                 one the sample is step 2's uniform point.  c_min == 0 takes step 2.  (A free direct motion has status 1 and is
 *                 never sampled.)  These steps are fp32 with the device's logf, sincospif and powf: they agree with an fp64
 *                 restatement to rounding, not bit for bit
 *   A problem that is not running gets its start row nodes[r, 0, :].  A goal_node outside -1 .. cap - 1 (the caller's error) is
 *   sampled as in step 2 and nothing is read there.
 * info [R, P] int32 (may be NULL): -1 not running, 0 uniform, 1 goal, 2 + t informed and accepted at try t, 2 + tries informed
 *   and fallen back to the uniform point.
 * Wrapped joints: the ellipsoid is the one around the shortest-arc image of the goal.  Every point of it satisfies the bound
 *   under the torus metric, because the wrapped sum is at most the unwrapped one; routes through other images of the goal are
 *   left to uniform_mix.
 * dcx_rrtstar_sample draws round `round` for the R problems of `state` on `device`, without a model (as
 *   dcx_rrtstar_extract_paths): one launch on the caller's stream; it reads nodes, cost, status and goal_node of the state.
 * dcx_rrtstar_run_sampled enqueues T rounds g = round0 .. round0 + T - 1: per round the sample launch on the state as the round
 *   finds it, then exactly the launches of dcx_rrtstar_run's round towards those rows - one round, shared by both calls.  With
 *   samples_out [T, R, P, dof] (and info_out [T, R, P]) the rounds' samples (and info words) are written there; otherwise the
 *   rows live in the work slot.  Capturable: no allocation, no synchronisation, nothing read back; equal seeds give equal bits,
 *   and T rounds in one call equal T calls of one round each.  `opts`, `margin`: dcx_rrtstar_run's.
 * work: dcx_rrtstar_sampled_work_bytes(model, R, slots, near) bytes: dcx_rrtstar_work_bytes' total, then one round's sample rows
 *   [R, P, dof].  dcx_rrtstar_work_bytes itself is unchanged.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL sample_opts; with R > 0 a NULL limits, state, nodes, cost,
 *   status, goal_node, goals or (dcx_rrtstar_sample) samples; tries outside 1 .. DCX_RRTSTAR_MAX_TRIES; goal_bias or uniform_mix
 *   outside [0, 1] or NaN; an unknown mode; a reserved field not 0; dcx_rrtstar_sample: R < 0, round < 0 or above 2^31 - 1, slots
 *   outside 1 .. DCX_RRT_MAX_SLOTS, cap outside 1 .. DCX_RRTSTAR_MAX_CAP, dof outside 1 .. DCX_MAX_DOF, a wrap_mask bit at or
 *   above dof; dcx_rrtstar_run_sampled: every error of dcx_rrtstar_run, and slots, cap, dof or wrap_mask that differ from opts'
 *   or the model's.  More than DCX_RRTSTAR_SAMPLE_MAX_PROBLEMS problems (the slot word r * 16 + p has 32 bits) is
 *   DCX_ERR_UNSUPPORTED.  R = 0 (or T = 0) launches nothing; dcx_rrtstar_sampled_work_bytes is 0 for arguments the call refuses. */
#define DCX_RRTSTAR_MAX_TRIES 16
#define DCX_RRTSTAR_SAMPLE_UNIFORM 0
#define DCX_RRTSTAR_SAMPLE_INFORMED 1
#define DCX_RRTSTAR_SAMPLE_MAX_PROBLEMS (1 << 28)
typedef struct dcx_rrtstar_sample_opts {
    const float* limits;   /* device [dof, 2]: lo_j, hi_j                                                   */
    uint64_t seed;         /* the Philox key                                                                */
    float    goal_bias;    /* in [0, 1]: the chance of the goal row while the problem has no goal node      */
    float    uniform_mix;  /* in [0, 1]: the chance of a uniform sample once it has one (mode informed)     */
    int32_t  mode;         /* DCX_RRTSTAR_SAMPLE_UNIFORM or DCX_RRTSTAR_SAMPLE_INFORMED                     */
    int32_t  tries;        /* 1 .. DCX_RRTSTAR_MAX_TRIES: informed draws before the uniform fallback        */
    int32_t  slots;        /* P: dcx_rrtstar_opts' slots                                                    */
    int32_t  cap;          /* dcx_rrtstar_opts' cap                                                         */
    int32_t  dof;          /* the model's dof                                                               */
    int32_t  reserved0;    /* 0                                                                             */
    uint64_t wrap_mask;    /* dcx_rrtstar_opts' wrap_mask                                                   */
    int64_t  reserved[2];  /* 0                                                                             */
} dcx_rrtstar_sample_opts;
int dcx_rrtstar_sample(int device, const dcx_rrtstar_state* state, int64_t R, const float* goals,
                       const dcx_rrtstar_sample_opts* sample_opts, int64_t round, float* samples, int32_t* info, void* stream);
size_t dcx_rrtstar_sampled_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t near);
int dcx_rrtstar_run_sampled(const dcx_model* m, const dcx_rrtstar_state* state, int64_t R, const float* goals,
                            const dcx_rrtstar_sample_opts* sample_opts, int32_t T, int64_t round0, const dcx_rrtstar_opts* opts,
                            const float* margin, void* work, size_t work_bytes, float* samples_out, int32_t* info_out, void* stream);

/* ---- batched RRT*: clearance-weighted edge costs (added under DCX_VERSION 109) ---------------------------- */
/* The same planner under an objective a shortcutter cannot optimise: an edge costs its length times a factor that grows with the
 * peak score along it, so the tree prefers motions that keep away from the obstacle boundary.  The reference's
 * misc/rrt_star.py does this in score_dist, length * (1 + a penalty of the worst sample's score), and scripts/motion_planner.py
 * hands OMPL a custom motionCost.  The objective travels in a struct of its own and through entry points of its own:
 * dcx_rrtstar_opts, its reserved fields and dcx_rrtstar_run are unchanged.
 * The objective (mode DCX_RRTSTAR_COST_PEAK) of a directed edge a -> b of a batch submitted to dcx_motion_worst with the closed
 * max_step rule, max_samples, margin, wrap_mask of the options and no gradients; w = its worst, L = the motion calls' own length
 * bits of a -> b as "batched RRT*" step 1 forms them:
 *   free  <=>  w <= 0          (NaN, an edge over max_samples, is not free: what first_hit -2 is to dcx_rrtstar_run)
 *   pen = fmaxf(w + band, +0)  band >= 0: how far below the margin a peak starts to cost, in score units
 *   f   = 1 + gain * pen       gain >= 0
 *   C   = L * f                the edge's cost
 * every operation fp32 and rounded alone, never contracted.  The shape is score_dist's with a hinge where the reference has exp:
 * with a hinge each step is one correctly rounded operation that a host referee reproduces, so the two agree bit for bit; an expf
 * would agree to rounding only.  free is dcx_check_motions_ex's verdict on the same batch (dcx_motion_worst documents that).
 * The round keeps dcx_rrtstar_run's numbering, its phases 1 (up to the check), 2, 4 and 6, its state and its fixed batches.  elen
 * holds C (the edge's cost, no longer its length); cost[i] = cost[parent[i]] + elen[i] as before.
 *   sweeps        - the three batches (R * P, R * P * K, R * P * K edges in (r, p[, j]) order, idle places nodes[r, 0] ->
 *                   nodes[r, 0]) go through dcx_motion_worst in place of dcx_check_motions_ex; one worst array per batch
 *   extend        - a slot is a candidate where its edge is free;  C0 = L0 * f(w0),  c0 = cost[near] + C0
 *   choose parent - place (r, p, j) submits u_j -> x where the lower bound (bits(cost[u_j] + Lj), u_j) < (bits(c0), near).  After
 *                   the sweep Cj = Lj * f(wj), cj = cost[u_j] + Cj: the parent is the free submitted u_j with the least
 *                   (bits(cj), u_j) that is still < (bits(c0), near); without one it is near, with C0 and c0
 *   rewire        - place (r, p, j) submits x -> v where the lower bound cost[x] + L' < cost[v].  After the sweep C' = L' * f(w'),
 *                   c' = cost[x] + C': the place stays in only where it is free and c' < cost[v]; the least (bits(c'), p) per v
 *                   wins and sets parent[v] = x, elen[v] = C'
 * The pruning by the lower bounds is exact: f >= 1 and fp32 products and sums are monotone, so C >= L and cost + C >= cost + L in
 * bits; a place the bound leaves out could not have won.  gain == 0 gives f == 1 and C == L bit for bit: the submissions, verdicts
 * and state are dcx_rrtstar_run's own.  No node's cost ever rises and the parent graph stays a tree (the rewire test is still
 * strict), and the set of nodes still does not depend on the parents.
 * Status 1 (the caller's, when it initialises the state): a free direct motion is the optimum only where its C has L's bits.  A
 * caller seeds a free but penalised direct motion as node 1 = goal with elen = cost = C, goal_node = 1, first_round -1 and status
 * 0: the problem keeps improving on it.
 * dcx_rrtstar_run_sampled_cost: dcx_rrtstar_run_sampled's sample launch in front of every round.  The informed sampler reads
 *   state.cost as it does there; its set d(start, x) + d(x, goal) <= c_best stays admissible because C >= L: a path through a
 *   point outside it is longer than c_best and therefore costs more.
 * Launches on the caller's stream only, no allocation, no synchronisation, no atomic decides any order, nothing read back: the
 *   calls can be captured; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.
 * work: dcx_rrtstar_cost_work_bytes / dcx_rrtstar_sampled_cost_work_bytes: dcx_rrtstar_work_bytes' layout with
 *   dcx_motion_worst_work_bytes of the larger batch at its head, then the batches' worst arrays and the slots' C0 and c0.
 * Argument errors: those of dcx_rrtstar_run (dcx_rrtstar_run_sampled); and DCX_ERR_INVALID for NULL cost_opts, an unknown mode,
 *   gain or band negative or NaN, a reserved field not 0 - all before any device work.  max_samples above 2^24 - 1 and a feature
 *   width without a worst-sample kernel are DCX_ERR_UNSUPPORTED.  The size queries are 0 for arguments the calls refuse.      */
#define DCX_RRTSTAR_COST_PEAK 1
typedef struct dcx_rrtstar_cost_opts {
    int32_t mode;         /* DCX_RRTSTAR_COST_PEAK, the only mode                                           */
    float   gain;         /* >= 0: the cost factor's slope per score unit of the hinge                      */
    float   band;         /* >= 0: how far below the margin a peak starts to cost                           */
    int32_t reserved0;    /* 0                                                                              */
    int64_t reserved[2];  /* 0                                                                              */
} dcx_rrtstar_cost_opts;
size_t dcx_rrtstar_cost_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t near);
int dcx_rrtstar_run_cost(const dcx_model* m, const dcx_rrtstar_state* state, int64_t R, const float* goals, const float* samples,
                         int32_t T, int64_t round0, const dcx_rrtstar_opts* opts, const dcx_rrtstar_cost_opts* cost_opts,
                         const float* margin, void* work, size_t work_bytes, void* stream);
size_t dcx_rrtstar_sampled_cost_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t near);
int dcx_rrtstar_run_sampled_cost(const dcx_model* m, const dcx_rrtstar_state* state, int64_t R, const float* goals,
                                 const dcx_rrtstar_sample_opts* sample_opts, int32_t T, int64_t round0, const dcx_rrtstar_opts* opts,
                                 const dcx_rrtstar_cost_opts* cost_opts, const float* margin, void* work, size_t work_bytes,
                                 float* samples_out, int32_t* info_out, void* stream);

/* ---- batched path shortcutting and RRT path extraction (added under DCX_VERSION 109) ---------------------- */
/* R piecewise-straight paths simplified in lockstep, P = opts->slots shortcut attempts per path and round: try the straight
 * motion between two waypoints and cut out what lies between (the path simplifier a planner's user expects before the paths go
 * to the optimisers; the reference's scripts/motion_planner.py gets it from OMPL).  All path logic runs on the device, the edge
 * checks are dcx_check_motions_ex's own launches, and nothing is read back between rounds.
 * State (dcx_shortcut_state; caller-owned device memory, R paths, W = opts->W):
 *   path [R, W, dof] float          row k < count[r] is waypoint k of path r
 *   count [R] int32                 0 .. W: the path's waypoints (a count above W is the caller's error: read as W)
 *   accepted [R] int32              shortcuts applied so far (the call adds to it)
 * Round t = 0 .. T - 1, path r, slot p < P, n = count[r] as it stands at the start of the round:
 *   1. pick, with (u0, u1) = draws[t, r, p, :]: the slot is idle if n < 3 or if either draw fails u >= 0 && u < 1 (a NaN fails
 *      it).  Otherwise, in fp32 with each operation rounded alone and the cast truncating:
 *        i = min((int)(u0 * (float)(n - 2)), n - 3),  m = n - 2 - i,  j = i + 2 + min((int)(u1 * (float)m), m - 1)
 *      so 0 <= i, i + 2 <= j <= n - 1
 *   2. check: the edge path[r, i] -> path[r, j] is checked by dcx_check_motions_ex (the closed max_step rule, opts->max_samples,
 *      margin, wrap_mask): first_hit == -1 makes the slot free, anything else (-2 included) rejects it
 *   3. apply: slots are taken in ascending order.  A free slot p is applied iff every already applied slot q of this round and
 *      path satisfies j_p <= i_q || j_q <= i_p (the interiors are disjoint and the intervals do not cross; an exact duplicate
 *      therefore loses)
 *   4. compact: waypoint k survives iff no applied (i, j) has i < k < j.  Survivors keep their order and their bits and move to
 *      index k - sum over the applied (i, j) with j <= k of (j - i - 1).  count[r] becomes the number of survivors, accepted[r]
 *      grows by the number of applied slots, rows at and beyond the new count are unspecified; path[r, 0] and
 *      path[r, count - 1] never change
 * Fixed batch: every round submits exactly R * P edges in (r, p) order.  An idle slot submits path[r, 0] -> path[r, 0] (one
 *   sample, its verdict ignored; that row must be readable even for count[r] == 0), so the geometry of the motion sweep never
 *   depends on the state: the call can be captured, and a referee that submits the same batch to dcx_check_motions_ex gets the
 *   same verdicts.
 * dcx_path_shortcut_run enqueues T rounds on the caller's stream: per round one pick launch, the launches of
 *   dcx_check_motions_ex, one commit launch.  No allocation, no synchronisation, no atomic decides any order, nothing read
 *   back; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.
 *   draws [T, R, P, 2] device floats;  margin [C] device floats, NULL = 0.
 * work: dcx_path_shortcut_work_bytes(model, R, slots) bytes of device memory, the caller's (dcx_check_motions' workspace for
 *   R * P edges, then the per-slot scratch: the edge batch qa and qb, first_hit and the picks); initialised by the call itself.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL model / opts; NULL state, state pointer, draws (T > 0) or
 *   work with R > 0; R < 0 or T < 0; max_step <= 0 or NaN; max_samples < 1; slots outside 1 .. DCX_SHORTCUT_MAX_SLOTS; W outside
 *   1 .. DCX_SHORTCUT_MAX_WAYPOINTS; a wrap_mask bit at or above dof; a reserved field not 0; work_bytes below
 *   dcx_path_shortcut_work_bytes.  R * slots above 2^31 - 1, R * slots * max_samples too large for one launch, dof above
 *   DCX_MAX_DOF and a feature width without a motion kernel are DCX_ERR_UNSUPPORTED.  R = 0 or T = 0 launches nothing.
 *   dcx_path_shortcut_work_bytes is 0 for arguments the call refuses.                                                        */
#define DCX_SHORTCUT_MAX_SLOTS 16
#define DCX_SHORTCUT_MAX_WAYPOINTS 65536
typedef struct dcx_shortcut_state {
    float*   path;          /* [R, W, dof]                                                                  */
    int32_t* count;         /* [R]: 0 .. W                                                                  */
    int32_t* accepted;      /* [R]: shortcuts applied so far (the call adds to it)                          */
} dcx_shortcut_state;
typedef struct dcx_shortcut_opts {
    float    max_step;     /* > 0: the sampling stride of every edge check                                  */
    int32_t  max_samples;  /* >= 1: an edge needing more samples is rejected; it sizes the sweep launches   */
    int32_t  slots;        /* P, 1 .. DCX_SHORTCUT_MAX_SLOTS                                                */
    int32_t  W;            /* rows per path, 1 .. DCX_SHORTCUT_MAX_WAYPOINTS                                */
    uint64_t wrap_mask;    /* bit j: coordinate j is an angle, walked along the shortest arc                */
    int64_t  reserved[2];  /* 0                                                                             */
} dcx_shortcut_opts;
size_t dcx_path_shortcut_work_bytes(const dcx_model* m, int64_t R, int32_t slots);
int dcx_path_shortcut_run(const dcx_model* m, const dcx_shortcut_state* state, int64_t R, const float* draws, int32_t T,
                          const dcx_shortcut_opts* opts, const float* margin, void* work, size_t work_bytes, void* stream);
/* The solved paths of a dcx_rrt_state as rows of path [R, W, dof], one launch on `device`, without a model.
 *   status[r] == 1: the path is tree 0 from its root to link[r, 0], then tree 1 from link[r, 1] to its root, n waypoints (a
 *     direct solve, link = (0, 0), is [start, goal]).  n <= W writes them to path[r, 0 .. n - 1] and sets count[r] = n; n > W
 *     leaves the row untouched and sets count[r] = -n, so W = 0 (path may then be NULL) is the size query.
 *   status[r] != 1: count[r] = 0.
 *   Each walk is bounded by cap hops: a chain that leaves 0 .. cap - 1 or does not reach parent -1 by then gives count[r] = 0,
 *     and nothing is read out of bounds.
 * Argument errors (DCX_ERR_INVALID): R < 0; cap outside 1 .. DCX_RRT_MAX_CAP; dof < 1; W < 0; with R > 0 a NULL state, nodes,
 *   parent, status, link or count, or a NULL path with W > 0.  R above 2^31 - 1 is DCX_ERR_UNSUPPORTED.  R = 0 launches
 *   nothing.                                                                                                                 */
int dcx_rrt_extract_paths(int device, const dcx_rrt_state* state, int64_t R, int32_t cap, int32_t dof,
                          float* path, int32_t* count, int32_t W, void* stream);

/* Partial shortcuts: the second mode, between points INSIDE segments (what OMPL's path simplifier does along a path).  The vertex
 * mode above can only join two waypoints: it removes vertices and never cuts a corner, so a three-waypoint path around an
 * obstacle is its fixed point.  Here a slot draws two arc-length positions on the path, checks the straight motion between the
 * two points and, where it is free, replaces everything between them by that chord.  State and opts are dcx_shortcut_state and
 * dcx_shortcut_opts as above; W is also the capacity a path may grow into (a slot inside two neighbouring segments adds a row).
 * Round t = 0 .. T - 1, path r, n = min(count[r], W) as it stands at the start of the round; fp32, each operation rounded alone
 * unless said otherwise:
 *   1. arc length: len_e (e = 0 .. n - 2) and c_e (e = 0 .. n - 1) are exactly dcx_path_resample's (below): the wrapped deltas,
 *      the squares summed from +0 in coordinate order, a correctly rounded sqrt, and its fixed association - chunks of
 *      DCX_RESAMPLE_CHUNK, the chunk totals added in order.  L = c_{n-1}.  Every slot of the path is idle if n < 3 or
 *      !(L > 0 && L < inf) (a NaN fails it).
 *   2. pick, with (u0, u1) = draws[t, r, p, :]: the slot is idle if either draw fails u >= 0 && u < 1.  Otherwise s0 = u0 * L,
 *      s1 = u1 * L, sa = min(s0, s1), sb = max(s0, s1), and for s in (sa, sb) the point at s is located as dcx_path_resample
 *      locates an output waypoint, word for word: e = the largest index in 0 .. n - 2 with c_e <= s; a = s - c_e; if
 *      !(a < len_e) the point takes the bits of path[r, e + 1]; else f = a / len_e, correctly rounded, and coordinate j is
 *      wrap2pi(q + f * d) on masked coordinates (product and sum rounded alone) and fma(f, d, q) elsewhere, q = path[r, e, j]
 *      and d the segment's wrapped delta.  That gives (ea, xa) and (eb, xb), ea <= eb.  ea == eb idles the slot: a chord inside
 *      one straight segment gains nothing.
 *   3. check: the edge xa -> xb is checked by dcx_check_motions_ex (the closed max_step rule, opts->max_samples, margin,
 *      wrap_mask): first_hit == -1 makes the slot free, anything else (-2 included) rejects it.
 *   4. apply: slots are taken in ascending order, with a running count cnt that starts at n.  A free slot p is applied iff every
 *      already applied slot q of this round and path satisfies eb_p < ea_q || eb_q < ea_p (no segment is shared) and
 *      cnt + 2 - (eb_p - ea_p) <= W; cnt then takes that value.  A slot with eb = ea + 1 grows the path by one row, every other
 *      slot keeps or shrinks it.
 *   5. rewrite: with the applied slots in path order 1, 2, ..., the new path is waypoints 0 .. ea_1, then xa_1, xb_1, waypoints
 *      eb_1 + 1 .. ea_2, then xa_2, xb_2, and so on up to waypoint n - 1.  Surviving waypoints keep their bits; waypoint k moves
 *      to index k + sum over the applied (ea, eb) with eb < k of (2 - (eb - ea)).  path[r, 0] and path[r, last] never change
 *      (ea >= 0 and eb + 1 <= n - 1).  count[r] = cnt, accepted[r] grows by the number of applied slots, rows at and beyond the
 *      new count are unspecified.
 * Only the new middle edge is checked.  The two end pieces path[ea] -> xa and xb -> path[eb + 1] lie on segments the path
 *   already had, but their max_step samples are not the old segment's samples, and xa, xb are rounded points beside, not on, the
 *   old segment: a path whose every segment passed the check may hold an end piece that does not.  The call promises no more
 *   than OMPL's simplifier does; a caller who needs every segment checked checks the final paths once.
 * Fixed batch: every round submits exactly R * P edges in (r, p) order, an idle slot path[r, 0] -> path[r, 0], as above.
 * dcx_path_shortcut_partial_run enqueues T rounds on the caller's stream: per round one pick launch, the launches of
 *   dcx_check_motions_ex, one commit launch.  No allocation, no synchronisation, no atomic decides any order, nothing read
 *   back; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.  draws and margin as
 *   above.
 * work: dcx_path_shortcut_partial_work_bytes(model, R, slots, W) bytes of device memory, the caller's (the vertex mode's
 *   workspace, then a [R, W, dof] stage for the rewritten rows and, for W above what a block's LDS holds, c and len [R, W]);
 *   initialised by the call itself.
 * Argument errors: as dcx_path_shortcut_run's, with work_bytes below dcx_path_shortcut_partial_work_bytes.  R = 0 or T = 0
 *   launches nothing.  dcx_path_shortcut_partial_work_bytes is 0 for arguments the call refuses (W outside
 *   1 .. DCX_SHORTCUT_MAX_WAYPOINTS among them) and non-decreasing in R, slots and W.                                        */
size_t dcx_path_shortcut_partial_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t W);
int dcx_path_shortcut_partial_run(const dcx_model* m, const dcx_shortcut_state* state, int64_t R, const float* draws, int32_t T,
                                  const dcx_shortcut_opts* opts, const float* margin, void* work, size_t work_bytes, void* stream);

/* Path shortcuts under the clearance objective: both modes above with a round that prices what it removes against what it
 * inserts and keeps a chord only if it costs less.  The length modes skim the obstacle boundary - they optimise length alone; here
 * a chord that runs closer to an obstacle than the corner it cuts is turned down.  The objective is "batched RRT*:
 * clearance-weighted edge costs"' own and travels in its struct, dcx_rrtstar_cost_opts, with its validation (mode
 * DCX_RRTSTAR_COST_PEAK, gain >= 0, band >= 0, reserved fields 0): an edge submitted to dcx_motion_worst with the closed max_step
 * rule, max_samples, margin and wrap_mask of the options and no gradients, w = its worst, L = the motion calls' own length bits
 * (wrapped deltas, squares summed from +0 in coordinate order, a correctly rounded sqrt), is free iff w <= 0 and costs
 *   C = L * (1 + gain * fmaxf(w + band, +0))
 * every operation fp32 and rounded alone, never contracted.  dcx_path_shortcut_run, dcx_path_shortcut_partial_run, their state, their
 * options and their workspaces are unchanged.
 * State: dcx_shortcut_state, and one more caller-owned device array
 *   seg [R, W] float                for k < count[r] - 1 the cost of segment k -> k + 1; entries at and beyond count[r] - 1 are
 *                                   unspecified
 * which the caller initialises from ONE dcx_motion_worst call on the consecutive waypoint pairs (same rule, max_samples, margin,
 * wrap_mask, no gradients): seg = C where the segment is free, +inf where it is not (w > 0, or NaN for a segment over max_samples).
 * An unfree segment therefore costs more than any free replacement: the rounds repair a path as well as improve it.  A NaN in seg
 * is the caller's error; no slot whose removed span holds one is applied (C < old is false).
 * The bits of a seg entry are those of the batch that priced it.  dcx_motion_worst derives its launch geometry from the batch's
 * size and max_samples, and on models large enough for that to change how a score is summed, the same edge swept in a batch of
 * another size can answer a peak a few units in the last place away.  An entry is thus, bit for bit, the price of its segment
 * swept in a batch of the size of the call that formed seg or of a round's batch (R * P, R * P * 3 edges) under the same
 * max_samples - which of the two, the rounds decide; a referee that submits the same batches gets the same bits.
 * Vertex mode, dcx_path_shortcut_run_cost; round t, path r, slot p:
 *   1. pick: dcx_path_shortcut_run's step 1, word for word: the same draws give the same (i, j), an idle slot (-1, -1).
 *   2. sweep: the R * P edges path[r, i] -> path[r, j] in (r, p) order go through dcx_motion_worst; an idle slot submits
 *      path[r, 0] -> path[r, 0].  A fixed batch: the launch geometry does not depend on the state.
 *   3. price: w = the edge's worst; the slot is free iff w <= 0.  C as above.  old = seg[i] + seg[i + 1] + ... + seg[j - 1], added
 *      in ascending order starting from seg[i].  The slot is gainful iff it is free and C < old (strict: a NaN fails it).
 *   4. apply: slots are taken in ascending order; a gainful slot is applied iff it satisfies step 3's disjointness rule of
 *      dcx_path_shortcut_run against every slot already applied: j_p <= i_q || j_q <= i_p.
 *   5. compact: the waypoints move exactly as in dcx_path_shortcut_run's step 4, and seg with them: segment k survives iff both its
 *      ends survive and it is not the i of an applied slot, and moves to the new index of waypoint k; the segment at the new index
 *      of an applied i takes that slot's C.  count and accepted as there.
 * Partial mode, dcx_path_shortcut_partial_run_cost: steps 1 and 2 (arc length, pick) are dcx_path_shortcut_partial_run's, word for
 * word, and give (ea, xa), (eb, xb).  Then
 *   3. sweep: three edges per slot, R * P * 3 in (r, p, piece) order: piece 0 path[ea] -> xa, piece 1 xa -> xb, piece 2
 *      xb -> path[eb + 1]; an idle slot submits path[r, 0] -> path[r, 0] three times.
 *   4. price: new = (C0 + C1) + C2; old = seg[ea] + ... + seg[eb], ascending from seg[ea].  The slot is gainful iff all three pieces
 *      are free and new < old.  A zero-length piece (xa with the bits of a waypoint) prices as L = 0, C = 0 and is free iff the
 *      score at that point is <= 0.
 *   5. apply and rewrite: dcx_path_shortcut_partial_run's steps 4 and 5 (no shared segment, the capacity bound, slot order) with
 *      "gainful" for "free".  seg is rewritten with the rows: a surviving segment moves with its first waypoint, the three new
 *      segments take C0, C1, C2 at the new indices of ea, xa and xb.
 *   All three pieces are swept and priced, so what "Only the new middle edge is checked" says of the length mode does not hold
 *   here: a path whose seg is finite keeps every segment free under the sweep that priced it.
 * gain == 0 gives C == L bit for bit.  The rounds are still not the length modes': those apply every free chord, these apply only
 *   chords with C < old - the never-lengthening variant (a free chord between two points of a polyline is never longer than the
 *   polyline in exact arithmetic, but the length modes also apply one that ties, or loses by a rounding, or replaces unfree
 *   segments; here the comparison decides).
 * Both calls enqueue T rounds on the caller's stream: per round one pick launch, the launches of dcx_motion_worst, one
 *   price-and-commit launch.  No allocation, no synchronisation, no atomic decides any order, nothing read back: the calls can be
 *   captured; repeated calls give the same bits, and T rounds in one call equal T calls of one round each.  draws and margin as
 *   dcx_path_shortcut_run's.
 * work: dcx_path_shortcut_cost_work_bytes(model, R, slots) / dcx_path_shortcut_partial_cost_work_bytes(model, R, slots, W) bytes
 *   of device memory, the caller's: dcx_motion_worst_work_bytes of the batch (R * slots, R * slots * 3 edges) at the head, then
 *   the edge batch, its worst and worst_idx, the pieces' L and the picks; the partial mode adds the [R, W, dof] stage of the
 *   rewritten rows, the [R, W] stage of their seg and, for W above what a block's LDS holds, c and len [R, W].  Both are 0 for
 *   arguments the calls refuse and non-decreasing in their arguments.
 * Argument errors, all before any device work: everything dcx_path_shortcut_run (dcx_path_shortcut_partial_run) refuses, with
 *   work_bytes below the size query of the call; DCX_ERR_INVALID for NULL seg with R > 0, for NULL cost_opts, an unknown mode, gain
 *   or band negative or NaN, a reserved field of it not 0.  max_samples above 2^24 - 1, a feature width without a worst-sample
 *   kernel and more than 2^31 - 1 swept edges per round are DCX_ERR_UNSUPPORTED.  R = 0 or T = 0 launches nothing.             */
size_t dcx_path_shortcut_cost_work_bytes(const dcx_model* m, int64_t R, int32_t slots);
int dcx_path_shortcut_run_cost(const dcx_model* m, const dcx_shortcut_state* state, float* seg, int64_t R, const float* draws, int32_t T,
                               const dcx_shortcut_opts* opts, const dcx_rrtstar_cost_opts* cost_opts, const float* margin, void* work,
                               size_t work_bytes, void* stream);
size_t dcx_path_shortcut_partial_cost_work_bytes(const dcx_model* m, int64_t R, int32_t slots, int32_t W);
int dcx_path_shortcut_partial_run_cost(const dcx_model* m, const dcx_shortcut_state* state, float* seg, int64_t R, const float* draws,
                                       int32_t T, const dcx_shortcut_opts* opts, const dcx_rrtstar_cost_opts* cost_opts,
                                       const float* margin, void* work, size_t work_bytes, void* stream);

/* ---- roadmap queries (added under DCX_VERSION 109) -------------------------------------------------------- */
/* Shortest paths over a roadmap for Q start/goal pairs at once: synchronous min-plus relaxation in fp32 without atomics
 * (dcx_sssp_run), then the routes as rows of one [Q, W, dof] tensor (dcx_sssp_extract_paths), on `device`, without a model.
 * Graph (dcx_graph; caller-owned device memory): the roadmap as a symmetric CSR
 *   rowptr [N + 1] int32, col [nnz] int32, weight [nnz] float
 *   Every row is sorted by col, each neighbour appears once, there are no self loops, and an entry (v, u, w) has its mirror
 *   (u, v, w).  Weights are lengths: >= 0, possibly +inf, never NaN.  The calls do NOT check any of this.  Memory safety alone
 *   is kept: a row's range is clipped to 0 .. nnz and an entry whose col lies outside 0 .. N - 1 is skipped.
 * State (dcx_sssp_state; caller-owned device memory), for Q independent queries:
 *   dist [2, N, Q] float     two buffers, node-major and query-minor: dist[b][v][q]
 *   pred [N, Q] int32        the node the current dist[v][q] was reached from, -1 for none
 * Round 0 (initialisation): query q has up to k start links (links->idx[q, s], links->len[q, s]), s < k.  An index of -1 means
 *   no link (as does any index outside 0 .. N - 1); the real indices of one query are distinct.  dist[0][v][q] is the link's
 *   length where v is linked and +inf elsewhere, dist[1] is +inf everywhere, pred is -1 everywhere.  changed is 1 iff any
 *   link of any query is real.
 * Round t >= 1 reads dist[(t - 1) & 1] only (dist_old) and writes dist[t & 1] (dist_new).  For node v and query q:
 *   cand = min over the entries e of row v, in row order, of (dist_old[col_e][q] + weight_e), each sum a single rounded fp32 add
 *   u    = the col of the first entry that attains the minimum
 *   cand < dist_old[v][q]:  dist_new[v][q] = cand and pred[v][q] = u
 *   otherwise:              dist_new[v][q] = dist_old[v][q] and pred[v][q] is untouched (an inf or NaN candidate never wins)
 *   pred changes on a strict decrease only, so the predecessor walks end at a linked node within N steps, zero-length edges
 *   and weights absorbed by rounding included; fp32 addition is monotone, so the fixed point is unique: that of a Dijkstra
 *   accumulating in fp32 from the links.
 * dcx_sssp_run enqueues rounds round0 .. round0 + n_rounds - 1 on the caller's stream; links is read when round0 == 0 only.
 *   changed [n_rounds] device int32: the call zeroes it, then changed[t - round0] = 1 is stored (a plain store) by whoever
 *   changed a (v, q) in round t.  A round whose predecessor INSIDE THE SAME CALL has changed == 0 returns at once: both buffers
 *   are equal by then.  The state after round t does not depend on how the rounds are split over calls or on the launch
 *   geometry; once a round reports 0 every later round does, and dist[0] == dist[1].
 *   Launches: one that zeroes changed, then round 0 as a fill and a scatter and every later round as one launch (a wave per
 *   (node, 64 queries)).  No allocation, no synchronisation, no atomic, nothing read back: the call can be captured.
 * dcx_sssp_extract_paths, one launch, a wave per query; rounds_done >= 1 rounds have run and dist[(rounds_done - 1) & 1] is
 * read.  mode [Q] int32, starts / goals [Q, dof], nodes [N, dof], goal links as the start links, direct_len [Q]:
 *   mode 0 (an endpoint collides; any value but 1 and 2 is taken as 0): count = 0, length = +inf
 *   mode 1 (the direct motion is free): the path is (start, goal), n = 2, length = direct_len[q]
 *   mode 2: length = min over the goal slots s, in slot order, of (dist[idx[q, s]][q] + len[q, s]), the first slot attaining it
 *     wins; +inf (or no real slot) means no route: count = 0.  Otherwise pred is walked back from that node to -1, at most N
 *     steps (a walk that does not end by then, or leaves 0 .. N - 1: count = 0, length = +inf), and the path is start, the
 *     walk's nodes in forward order, goal: n = hops + 2 waypoints.  length is thus a float32 sum in path order.
 *   count[q] = n where the n waypoints fit in W and were written to path[q, 0 .. n - 1]; -n where n > W, the row left as it is:
 *   W = 0 (path may then be NULL) asks for the sizes alone.  length[q] is set either way.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL graph / state / links; a negative Q, N or nnz; k outside
 *   1 .. DCX_KNN_MAX_K; dof outside 1 .. 64; round0 < 0, n_rounds < 0, rounds_done < 1, W < 0; a reserved field not 0; with
 *   Q > 0 a NULL rowptr, dist, pred, changed (n_rounds > 0), link array (dcx_sssp_run: when round0 == 0), col or weight
 *   (nnz > 0), nodes (N > 0), mode, starts, goals, direct_len, count or length, or a NULL path with W > 0.  N, nnz or N * Q
 *   beyond int32 indexing and a grid beyond one launch are DCX_ERR_UNSUPPORTED.  Q == 0 returns 0 and touches nothing.       */
typedef struct dcx_graph {
    const int32_t* rowptr;   /* [N + 1]                                                                     */
    const int32_t* col;      /* [nnz]                                                                       */
    const float*   weight;   /* [nnz]                                                                       */
    int64_t  N, nnz;
    int64_t  reserved[2];    /* 0                                                                           */
} dcx_graph;
typedef struct dcx_sssp_state {
    float*   dist;           /* [2, N, Q]                                                                   */
    int32_t* pred;           /* [N, Q]                                                                      */
    int64_t  reserved[2];    /* 0                                                                           */
} dcx_sssp_state;
typedef struct dcx_sssp_links {
    const int32_t* idx;      /* [Q, k]: -1 = no link                                                        */
    const float*   len;      /* [Q, k]                                                                      */
    int64_t  reserved[2];    /* 0                                                                           */
} dcx_sssp_links;
int dcx_sssp_run(int device, const dcx_graph* graph, int64_t Q, const dcx_sssp_links* links, int32_t k,
                 const dcx_sssp_state* state, int32_t round0, int32_t n_rounds, int32_t* changed, void* stream);
int dcx_sssp_extract_paths(int device, const dcx_graph* graph, const float* nodes, int32_t dof, const dcx_sssp_state* state,
                           int32_t rounds_done, int64_t Q, int32_t k, const int32_t* mode, const float* starts, const float* goals,
                           const dcx_sssp_links* goal_links, const float* direct_len, float* path, int32_t* count, float* length,
                           int32_t W, void* stream);

/* ---- lazy roadmap queries (added under DCX_VERSION 109) --------------------------------------------------- */
/* A roadmap whose edges are checked only when a shortest route uses them (lazy PRM): the relaxation above runs over ALL
 * candidate edges, dcx_sssp_mark_routes lists the still unchecked edges of the routes it found, ready for the motion checks, and
 * dcx_graph_apply_checks writes the verdicts back into the graph: a blocked edge's weight becomes +inf, which the relaxation
 * takes as "no edge" (an inf candidate never wins).  The caller repeats relax (from round 0: distances only grow when edges go,
 * so an earlier state is no valid start) - mark - check - apply until a mark pass lists nothing.  On `device`, without a model.
 * Edges (dcx_lazy_graph; caller-owned device memory) beside the CSR of a dcx_graph, M undirected edges with ids 0 .. M - 1:
 *   eid   [nnz] int32      CSR entry -> edge id
 *   ent   [M, 2] int32     edge id -> its two CSR entries (row ends[m, 0] and row ends[m, 1])
 *   ends  [M, 2] int32     edge id -> its two nodes
 *   state [M] uint8        0 unknown, 1 free, 2 blocked; any other value is read as "not unknown"
 *   The calls do NOT check that the three index arrays agree with the CSR or with each other.  Memory safety alone is kept: an
 *   index outside its range (an edge id outside 0 .. M - 1, an entry outside 0 .. nnz - 1, a node outside 0 .. N - 1) is skipped.
 * dcx_sssp_mark_routes; graph, nodes [N, dof], state, rounds_done, Q, k, mode and goal_links exactly as dcx_sssp_extract_paths
 * reads them (the graph's weight is not read).  For every query q:
 *   mode[q] != 2: pending[q] = 0.
 *   mode[q] == 2: the goal slot is dcx_sssp_extract_paths' (the first slot, in slot order, with the least dist + len, one rounded
 *     fp32 add); pred is walked back from that node to -1, at most N steps.  No real slot, a sum that is not below +inf, a walk
 *     that does not end by then or leaves 0 .. N - 1: no route, pending[q] = 0 and nothing is marked.  Otherwise, for every hop
 *     (v, u = pred[v][q]) of the walk, e = the first entry of row v (the row's range clipped to 0 .. nnz) whose col is u and
 *     m = eid[e]; where state[m] == 0 the edge is marked and counted in pending[q].  A hop without such an entry, or with m
 *     outside 0 .. M - 1, is skipped.  The links (start and goal) are no edges of the graph and are never marked.
 *   total = the number of marked edges (an edge on several routes counts once), n = min(total, capacity);
 *   n_out[0] = total, n_out[1] = n;  list[0 .. n - 1] = the n smallest marked edge ids in ascending order;
 *   qa[i] = nodes[ends[list[i], 0]] and qb[i] = nodes[ends[list[i], 1]] (the bits copied; an end that is no node leaves its row
 *   as it is).  Entries i >= n of list, qa and qb are left as they are; capacity = 0 (list, qa, qb may then be NULL) counts alone.
 *   pending [Q] int32, list [capacity] int32, qa / qb [capacity, dof] float, n_out [2] int32: device memory, written whatever
 *   they held.  Neither state nor the graph is written.
 *   work: dcx_sssp_mark_routes_work_bytes(M) bytes of device memory, 16-byte aligned, the caller's; initialised by the call
 *   itself (one mark byte per edge, zeroed first, and one offset per 16 edges).
 *   Launches: four (the marks zeroed; a wave per query making plain same-value stores into the marks; an ordered scan in one
 *   workgroup; a scatter).  No allocation, no synchronisation, no atomic, nothing read back: the call can be captured, and the
 *   same inputs give the same bits whatever the order the waves arrive in.
 * dcx_graph_apply_checks; list and n_out as dcx_sssp_mark_routes left them, hit [at least n_out[1]] uint8 the checker's
 * verdicts (non-zero = the motion collides).  n_out[1] is read on the device (values outside 0 .. M are clipped), so the host
 * needs no second read-back.  For i < n_out[1], m = list[i]:
 *   state[m] = hit[i] ? 2 : 1;  where hit[i]: weight[ent[m, 0]] = weight[ent[m, 1]] = +inf
 *   any_blocked [1] int32: the call zeroes it, then 1 is stored (a plain store) by whoever saw a hit.
 *   THE GRAPH'S weight IS WRITTEN, though dcx_graph declares it const: it must be memory the caller may change.  Nothing else of
 *   the graph is read.  Launches: two (the flag zeroed; a thread per listed edge, striding).  Capturable as above.
 * Argument errors (DCX_ERR_INVALID, before any device work): NULL graph / lazy / state / goal_links; a negative Q, N, nnz, M or
 *   capacity; k outside 1 .. DCX_KNN_MAX_K; dof outside 1 .. 64; rounds_done < 1; a reserved field not 0; with Q > 0 and M > 0
 *   (dcx_sssp_mark_routes) a NULL rowptr, col (nnz > 0), dist, pred (N > 0), nodes (N > 0), eid (nnz > 0), ent, ends, lazy
 *   state, mode, link array, pending or n_out, a NULL list, qa or qb with capacity > 0, a NULL or misaligned work or work_bytes
 *   below dcx_sssp_mark_routes_work_bytes(M); with M > 0 (dcx_graph_apply_checks) a NULL weight (nnz > 0), ent, lazy state,
 *   list, n_out, hit or any_blocked.  N, nnz, M or N * Q beyond int32 indexing and a grid beyond one launch are
 *   DCX_ERR_UNSUPPORTED.  Q == 0 or M == 0 returns 0 and touches nothing (no edge can be marked: the caller's total is 0).
 *   dcx_sssp_mark_routes_work_bytes is 0 for M outside 1 .. INT32_MAX and non-decreasing in M.                              */
typedef struct dcx_lazy_graph {
    const int32_t* eid;      /* [nnz]                                                                       */
    const int32_t* ent;      /* [M, 2]                                                                      */
    const int32_t* ends;     /* [M, 2]                                                                      */
    uint8_t*       state;    /* [M]: 0 unknown, 1 free, 2 blocked                                           */
    int64_t  M;
    int64_t  reserved[2];    /* 0                                                                           */
} dcx_lazy_graph;
size_t dcx_sssp_mark_routes_work_bytes(int64_t M);
int dcx_sssp_mark_routes(int device, const dcx_graph* graph, const dcx_lazy_graph* lazy, const float* nodes, int32_t dof,
                         const dcx_sssp_state* state, int32_t rounds_done, int64_t Q, int32_t k, const int32_t* mode,
                         const dcx_sssp_links* goal_links, int32_t* pending, int32_t* list, float* qa, float* qb, int64_t capacity,
                         int32_t* n_out, void* work, size_t work_bytes, void* stream);
int dcx_graph_apply_checks(int device, const dcx_graph* graph, const dcx_lazy_graph* lazy, const int32_t* list,
                           const int32_t* n_out, const uint8_t* hit, int32_t* any_blocked, void* stream);

/* ---- batched path resampling (added under DCX_VERSION 109) ------------------------------------------------ */
/* R piecewise-straight paths of uneven length resampled to T waypoints each, equally spaced in arc length under the motion
 * calls' metric: what joins the planners' paths (dcx_rrt_extract_paths, dcx_sssp_extract_paths, dcx_path_shortcut_run) to the
 * trajectory optimisers, which take rows of one fixed length.  One launch on `device`, without a model.
 *   path [R, W, dof] float, count [R] int32, wrap_mask: as for dcx_path_shortcut_run (a count above W is read as W)
 *   out [R, T, dof] float           the resampled rows; must not overlap path
 *   out_count [R] int32             T, or 0 for a row without a path
 *   length [R] float                the path's length L; may be NULL
 * Path r, n = min(count[r], W).  Every float operation is fp32 and rounded on its own unless said otherwise.
 * No path: n < 2 gives out_count[r] = 0 and length[r] = NaN, and row r of out is not written.
 * Segment lengths, e = 0 .. n - 2: d_e[j] = the delta of coordinate j of the motion path[r, e] -> path[r, e + 1] (the rounded
 *   difference, wrapped to the shortest arc where bit j of wrap_mask is set: dcx_check_motions_ex's), and len_e the edge length
 *   as the motion calls form it: the squares summed from +0 in coordinate order, product and sum rounded separately, then a
 *   correctly rounded square root.
 * Arc length at the waypoints, in a fixed association (a parallel implementation and a referee must add in the same order).
 *   Chunk g covers segments 32 g .. 32 g + 31 (DCX_RESAMPLE_CHUNK):
 *     within a chunk   p_{g,0} = +0,  p_{g,i+1} = p_{g,i} + len_{32 g + i};  the chunk total t_g is the last p of the chunk
 *     across chunks    b_0 = +0,  b_{g+1} = b_g + t_g, taken in order
 *     c_e = b_{e / 32} + p_{e / 32, e % 32} for e = 0 .. n - 1, and L = c_{n-1}
 *   c is non-decreasing: lengths are >= 0 and fp addition is monotone in each operand, so p grows within a chunk, b grows
 *   across chunks, and c_{32 g + 32} = b_g + t_g is not below any b_g + p_{g,i}.  The search below relies on it.
 * Bad length: !(L < +inf) (NaN or infinite) gives out_count[r] = 0 and length[r] = L, and the row is not written.  (Every NaN
 *   stored in length is the quiet NaN 0x7fc00000: which NaN an fp32 sum of NaNs yields is the hardware's choice.)
 * Otherwise out_count[r] = T, length[r] = L, out[r, 0] takes the bits of path[r, 0], out[r, T - 1] the bits of
 *   path[r, n - 1], and for 0 < t < T - 1:
 *     step = L / (float)(T - 1), correctly rounded;  s = (float)t * step
 *     e = the largest index in 0 .. n - 2 with c_e <= s (c_0 = 0 <= s: there is one), so zero-length segments are skipped and
 *         an s that rounding pushed past L lands in the last segment
 *     a = s - c_e
 *     !(a < len_e):  out[r, t] takes the bits of path[r, e + 1]
 *     else f = a / len_e, correctly rounded, and coordinate j is
 *         wrap2pi(path[r, e, j] + f * d_e[j]), product and sum rounded alone, where bit j of the mask is set
 *         fma(f, d_e[j], path[r, e, j]) elsewhere
 *       (the split the motion calls' samples make).
 * Launch behaviour: one call does no allocation and no synchronisation, no atomic decides any order, nothing is read back; it
 *   can be captured, and repeated calls give the same bits.
 * work: dcx_path_resample_work_bytes(R, W) bytes of device memory, the caller's (c and len of the rows too long for a block's
 *   LDS, [R, W] floats each); written by the call before it is read.
 * Argument errors (DCX_ERR_INVALID, before any device work): R < 0; W outside 1 .. DCX_SHORTCUT_MAX_WAYPOINTS; T outside
 *   2 .. DCX_SHORTCUT_MAX_WAYPOINTS; dof < 1; a wrap_mask bit at or above dof; with R > 0 a NULL path, count, out, out_count or
 *   work; work_bytes below dcx_path_resample_work_bytes.  R above 2^31 - 1 and dof above DCX_MAX_DOF are DCX_ERR_UNSUPPORTED.
 *   R = 0 launches nothing and accepts NULLs.  dcx_path_resample_work_bytes is 0 for a refused R or W, and non-decreasing in R
 *   and in W.                                                                                                                 */
#define DCX_RESAMPLE_CHUNK 32
size_t dcx_path_resample_work_bytes(int64_t R, int32_t W);
int dcx_path_resample(int device, const float* path, const int32_t* count, int64_t R, int32_t W, int32_t dof,
                      uint64_t wrap_mask, int32_t T, float* out, int32_t* out_count, float* length,
                      void* work, size_t work_bytes, void* stream);

/* ---- kernel-perceptron trainer (producer of the path's state) ----------------------- */
/* DiffCo.train_perceptron kernel_perceptrons.py:98-137 and MultiDiffCo.train_perceptron
 * deprecated/MultiDiffCo.py:50-83 as one persistent launch: worst-margin search, lazily filled kernel rows,
 * margin fix / support retirement, until convergence or max_iteration.
 *   feats [N, D] dev   transformed samples          y [N, C] dev   labels (normally -1 / +1; any other value
 *                 is used as given: margin y*h, target beta^((1+y)/2)*y, like the reference's expressions)
 *   gains, hypothesis [N, C] dev in/out (zeros for a cold start, previous state for a jump start)
 *   kernel_matrix [N, N] dev in/out: zeros = "row not computed yet"; row i AND column i are filled when sample i
 *                 is first selected (K[i, :] = K[:, i] = k(x_i, X), kernel_perceptrons.py:117-119), so the sub-block
 *                 over the kept supports is complete even for a sample that was never selected itself
 *   info [2] dev out: iterations used; 1 if converged, 0 if not, -1 if the multi-workgroup form gave up on a
 *                 grid barrier (another kernel kept its workgroups from running for seconds)
 * For one label column and N <= 131072 a register-resident kernel, which keeps a label as its sign, is used: one
 * workgroup up to N = 4096, beyond that N / 1024 workgroups on as many CUs (a cooperative launch, one grid-wide barrier
 * per iteration; the same argmin sequence, bit for bit).  Whether the labels really are -1 / +1 is checked by those
 * kernels themselves, on the device (any other label: the generic loop, which uses y as given) - like every entry
 * point of this library the call does not synchronise the caller's stream, and its one-workgroup form can be captured
 * in a HIP graph (a stream that is being captured never takes the multi-workgroup form).  After info[1] == -1 gains,
 * hypothesis and kernel_matrix have been partly updated in place: re-initialise them before running again, e.g. with
 * dcx_train_perceptron_ex(..., DCX_TRAIN_ONE_WORKGROUP, ...), which cannot give up.  Debug knob "train_grid": 0 = one
 * workgroup only, 1 = several from N = 2048, 2 = the generic one-workgroup kernel whatever the labels.            */
int dcx_train_perceptron(int device, int kernel_kind, const float* kparams, float beta, const float* feats, int64_t N,
                         int32_t D, const float* y, int32_t C, float* gains, float* hypothesis, float* kernel_matrix,
                         int32_t max_iteration, int32_t* info, void* stream);
/* the same with per-call flags (thread-safe, unlike the process-wide knob): DCX_TRAIN_ONE_WORKGROUP = never the
 * multi-workgroup form for this call                                                                          */
#define DCX_TRAIN_ONE_WORKGROUP 1
int dcx_train_perceptron_ex(int device, int kernel_kind, const float* kparams, float beta, const float* feats, int64_t N,
                            int32_t D, const float* y, int32_t C, float* gains, float* hypothesis, float* kernel_matrix,
                            int32_t max_iteration, int32_t* info, int32_t flags, void* stream);

/* ---- pieces of the path exposed on their own ---------------------------------------- */
/* X[b] = T(q_b): model.*.fkine (see DCX_FK_*).  q [B, dof] dev -> X [B, n_points*point_dim] dev */
int dcx_fkine(int device, const dcx_fk_desc* fk, const float* q, int64_t B, float* X, void* stream);
/* gq[b] = J_T(q_b)^T gX[b]  (autograd of fkine).  gX [B, D] dev -> gq [B, dof] dev          */
int dcx_fkine_vjp(int device, const dcx_fk_desc* fk, const float* q, const float* gX, int64_t B,
                  float* gq, void* stream);
/* Link transforms on their own - the two helpers user-written robot classes build their FK from (model.py:230, 437):
 *   dcx_dh_frames     utils.DH2mat utils.py:66-75: T[b, i] = Rz(theta) Tz(d_i) Tx(a_i) Rx(alpha_i), theta = q[b, i]
 *                     rows (c, -s ca, s sa, a c), (s, c ca, -c sa, a s), (0, sa, ca, d), (0, 0, 0, 1)
 *                     q [B, dof] dev; a, d, sin_alpha, cos_alpha [dof] dev -> T [B, dof, 4, 4] dev
 *   dcx_euler_frames  utils.euler2mat utils.py:15-38: R[b] = Rz(yaw) Ry(pitch) Rx(roll), phi[b] = (roll, pitch, yaw)
 *                     phi [B, 3] dev -> R [B, 3, 3] dev
 * and their autograd with respect to the angles: gq[b, i] = sum_rc gT[b, i, r, c] dT[b, i, r, c] / d q[b, i];
 * gphi[b, k] = sum_rc gR[b, r, c] dR[b, r, c] / d phi[b, k].  HBM-bound (64 B / 36 B written per frame).           */
int dcx_dh_frames(int device, const float* q, int64_t B, int32_t dof, const float* a, const float* d, const float* sin_alpha,
                  const float* cos_alpha, float* T, void* stream);
int dcx_dh_frames_vjp(int device, const float* q, int64_t B, int32_t dof, const float* a, const float* sin_alpha,
                      const float* cos_alpha, const float* gT, float* gq, void* stream);
int dcx_euler_frames(int device, const float* phi, int64_t B, float* R, void* stream);
int dcx_euler_frames_vjp(int device, const float* phi, const float* gR, int64_t B, float* gphi, void* stream);
/* K[b, j] = K(x_b, s_j): KernelFunc.__call__ kernel.py:17-29, 49-57, 73-79 (used by the trainer's
 * row fill kernel_perceptrons.py:117-119 and fit_poly :271-287).  x [B, D], s [S, D] dev -> K [B, S] dev */
int dcx_kernel_matrix(int device, int kernel_kind, const float* kparams, const float* x, int64_t B,
                      const float* s, int64_t S, int32_t D, float* K, void* stream);

/* ---- geometric ground truth (added under DCX_VERSION 109) -------------------------------------------------- */
/* A sphere model of the robot against a world of primitives: the true collision labels the proxy is trained on and verified
 * against, computed on the device.  The reference takes them from FCL / trimesh (ShapeEnv, collision_interfaces/
 * env_interface.py:35-122: Box, Sphere, Cylinder, Capsule by `extents` / `radius` / `height` and a 4x4 transform) through its
 * checkers (collision_checkers.py:28-125); meshes are not part of this library.
 *
 * The robot's spheres are the control points of `spheres_fk` (M = n_points <= DCX_MAX_POINTS, point_dim 2 or 3; 2 means z = 0)
 * with radii[k]; an obstacle is one 64-byte row: with the local point l = R^T (p - c),
 *   DCX_GEOM_SPHERE    p = (rho, -, -)          d = |l| - rho
 *   DCX_GEOM_BOX       p = half extents h       u = |l| - h (per axis);  d = |max(u, 0)| + min(max(u_x, u_y, u_z), 0)
 *   DCX_GEOM_CAPSULE   p = (rho, hl, -)         d = |l - (0, 0, clamp(l_z, -hl, hl))| - rho     (hl: half the axis segment, local z)
 *   DCX_GEOM_CYLINDER  p = (rho, hl, -)         a = hypot(l_x, l_y) - rho, b = |l_z| - hl;  d = min(max(a, b), 0) + |max((a, b), 0)|
 * type_group = DCX_GEOM_TYPE_GROUP(type, group); rt: the rows of R^T, row-major.
 *
 * clearance[b, g] = min over spheres k and obstacles o of group g of d_o(p_k(q_b)) - radii[k]; witness[b, g] = (o, k +
 * opt->sphere_base) of the first pair, in (obstacle, sphere) loop order, that attains it under a strict <.  A group without
 * obstacles (O = 0 as well) gives +inf and (-1, -1); rows whose group is outside [0, n_groups) or whose type is unknown are
 * ignored.  grad[b] = d min_g clearance[b, g] / d q_b: the unit normal of the witness pair's solid at the sphere's centre through
 * the transform's J^T, in the same launch; where the normal is undefined (|l| = 0 for a sphere or on a capsule's axis segment, a
 * point on a cylinder's axis, a box's medial planes) a fixed choice or zero, never NaN; zeros where there is no witness.
 * opt->accumulate = 1: clearance / witness / grad hold an earlier call's results for the same q and obstacles (another chunk of
 * the robot's spheres); an entry is overwritten only where this call's is strictly smaller, the gradient row only where this
 * call's overall minimum is strictly smaller than the one there.  Robots with more than DCX_MAX_POINTS spheres take one call
 * per chunk on one stream.
 * No allocation, no synchronisation, no atomics, nothing read back: capturable once `spheres_fk`'s program is on the device (the
 * first call with a description uploads it, as dcx_fkine).  DCX_ERR_INVALID: a NULL argument that is needed, B < 0, O < 0, a
 * reserved field not 0, n_groups outside [1, DCX_MAX_C], sphere_base < 0, accumulate not 0 / 1, a description whose points are
 * not 2- or 3-dimensional.  DCX_ERR_UNSUPPORTED: O above 2^31 - 1, a description whose block needs more than 64 KiB of LDS. */
#define DCX_GEOM_SPHERE 0
#define DCX_GEOM_BOX 1
#define DCX_GEOM_CAPSULE 2
#define DCX_GEOM_CYLINDER 3
#define DCX_GEOM_TYPE_GROUP(type, group) ((int32_t)(type) | ((int32_t)(group) << 8))
typedef struct dcx_geom_obstacle { int32_t type_group; float rt[9]; float c[3]; float p[3]; } dcx_geom_obstacle;   /* 64 bytes */
typedef struct dcx_geom_opts { int32_t n_groups, sphere_base, accumulate, reserved; } dcx_geom_opts;
/* stands in for ShapeEnv's collision queries (env_interface.py:35-122) as the checkers call them (collision_checkers.py:28-125) */
int dcx_geom_clearance(int device, const dcx_fk_desc* spheres_fk, const float* radii /*[M] device*/,
                       const dcx_geom_obstacle* obstacles /*[O] device*/, int64_t O, const float* q, int64_t B,
                       const dcx_geom_opts* opt, float* clearance /*[B, G]*/, int32_t* witness /*[B, G, 2] or NULL*/,
                       float* grad /*[B, dof] or NULL*/, void* stream);

/* x with A x = B: the S x S system fit_poly ends in (torch.linalg.solve at kernel_perceptrons.py:283, deprecated/DiffCo.py:162,
 * deprecated/MultiDiffCo.py:151 - add `reg` to A's diagonal first).  LU with partial pivoting in fp64, ONE launch.
 * A [n, n], B [n, nrhs] -> X [n, nrhs], all row-major fp32 on the device; 1 <= n <= DCX_SOLVE_MAX_N, 1 <= nrhs <= 64.
 * work: dcx_solve_work_bytes(n, nrhs) bytes of device memory, the caller's (no allocation, no synchronisation here; the
 * stream may be under capture).  info [2] int32 on the device: info[0] = 0, or k > 0 when the k-th pivot is exactly zero
 * (LAPACK's info; X is then not a solution), or -1 when a grid barrier gave up (another kernel held the CUs for seconds):
 * call again with DCX_SOLVE_ONE_WORKGROUP in flags.  */
#define DCX_SOLVE_MAX_N 4096
#define DCX_SOLVE_ONE_WORKGROUP 1
size_t dcx_solve_work_bytes(int64_t n, int64_t nrhs);
int dcx_solve(int device, const float* A, const float* B, int64_t n, int64_t nrhs, float* X, void* work, size_t work_bytes,
              int32_t* info, int32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCX_H */
