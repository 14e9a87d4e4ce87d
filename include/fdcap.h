/* fdcap.h -- C-ABI of libfdcap_hip.so: the MI355X (gfx950) hot path of
 * aptx4869lm/4DCapture-FPV `global_optimization.py` FittingOP.fitting(mode='global').
 *
 * The reference has no FFI layer; its boundary is three third-party Python operators plus the
 * optimiser loop around them.  Each entry point below names the reference
 * call site (file:line in /root/reference) it replaces.  Binding stub: INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch types; every `*_d` / "device" pointer is a caller-owned HIP device
 *     pointer (a torch tensor's storage), never freed or retained beyond the call unless the
 *     function says "registered";
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, nothing synchronises unless stated;
 *   - return value: 0 ok, negative FDCAP_E_* bad argument / state, positive = hipError_t;
 *   - one context per device per clip; calls on one context are serialised by the caller
 *     (the reference is single-threaded, single-stream);
 *   - fp32 everywhere (reference dtype: global_optimization.py:175,:185,:224,:707), int32 /
 *     int64 only for indices.
 */
#ifndef FDCAP_H
#define FDCAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDCAP_OK 0
#define FDCAP_E_ARG (-1)      /* null pointer / bad size */
#define FDCAP_E_STATE (-2)    /* call order (e.g. no scene registered) */
#define FDCAP_E_NODEVICE (-3) /* no HIP device visible */
#define FDCAP_E_COMM (-4)     /* RCCL not loadable, or an RCCL call failed: fdcap_comm_last_error() */
#define FDCAP_UNIQUE_ID_BYTES 128

#define FDCAP_NUM_JOINTS 55
#define FDCAP_XDIM 78         /* optimised row: transl3 6D6 betas10 latent32 lh12 rh12 camt3 */
#define FDCAP_PDIM 75         /* file row:      transl3 aa3 betas10 latent32 lh12 rh12 camt3 */
#define FDCAP_MAX_SCENE_POINTS 67000000   /* fdcap_set_scene refuses more (FDCAP_E_ARG): 32 B of MFMA fragments per point, 32-bit offsets */
#define FDCAP_MAX_SCENES 8    /* scene slots of a context (fdcap_set_scene_slot); slot 0 is fdcap_set_scene's */
#define FDCAP_NUM_LOSSES 8   /* rec, vposer, smoothing, contact, world_smoothing, total, reprojection (FDCAP_LOSS_REPROJ), 1 spare */
#define FDCAP_LOSS_REPROJ 6  /* slot of the clip-level reprojection term's partial sum (fdcap_opt_set_reproj); mode 'local''s second loop, which the
                              * term excludes, keeps its own use of the slot */

typedef struct fdcap_ctx fdcap_ctx;

/* Host arrays (copied to the device by fdcap_ctx_create).  Names follow the SMPL-X npz keys
 * read by smplx.create (global_optimization.py:154-168) and the VPoser v1 state-dict keys read
 * by load_vposer (:153). */
typedef struct fdcap_model_desc {
    int32_t num_verts;            /* V (10475 for SMPL-X) */
    const float* v_template;      /* [V,3] */
    const float* shapedirs;       /* [V,3,num_shape] first 10 = betas (num_betas=10, :156-159) */
    int32_t num_shape;            /* >= 10; columns >= 10 are expression (zero in the reference) */
    const float* posedirs;        /* [486, V*3] (library layout) */
    const float* J_regressor;     /* [55,V] */
    const int32_t* parents;       /* [55], root -1 */
    const float* lbs_weights;     /* [V,55] */
    const float* hands_componentsl; /* [12,45] first num_pca_comps=12 rows */
    const float* hands_componentsr; /* [12,45] */
    const float* hands_meanl;     /* [45] (flat_hand_mean=False) */
    const float* hands_meanr;     /* [45] */
    const float* vp_fc1_w;        /* bodyprior_dec_fc1.weight [512,32] */
    const float* vp_fc1_b;        /* [512] */
    const float* vp_fc2_w;        /* bodyprior_dec_fc2.weight [512,512] */
    const float* vp_fc2_b;        /* [512] */
    const float* vp_out_w;        /* bodyprior_dec_out.weight [126,512] */
    const float* vp_out_b;        /* [126] */
} fdcap_model_desc;

/* Optimiser configuration = fittingconfig / lossconfig (global_optimization.py:663-686) plus
 * the constants buried in fitting() (:564, :570, :582). */
typedef struct fdcap_opt_config {
    int32_t n_total;        /* frames in the whole clip (mean denominators) */
    int32_t n_local;        /* frames owned by this rank */
    int32_t frame0;         /* global index of the first owned frame */
    float lr;               /* init_lr_h = 0.005 (:671) */
    float weight_loss_rec;  /* 1 (:682) */
    float weight_loss_vposer; /* 0.001 (:683), logged only */
    float weight_contact;   /* 0.1 (:684) */
    float phase1_contact;   /* 0.1  (:570) */
    float phase1_smooth;    /* 1.0  (:570) */
    float phase2_world;     /* 1.0  (:582) */
    float phase2_smooth;    /* 0.5  (:582) */
    float scale_init;       /* 1.8  (:179) */
    int32_t legacy_zero_grad; /* 0: torch>=2 zero_grad(set_to_none=True) semantics */
} fdcap_opt_config;

/* ---- context ------------------------------------------------------------------------------ */
/* Replaces FittingOP.__init__'s model construction (global_optimization.py:153-171). */
int fdcap_ctx_create(const fdcap_model_desc* model, fdcap_ctx** out);
void fdcap_ctx_destroy(fdcap_ctx* ctx);
const char* fdcap_version(void);
/* "packed_fp32=off" for a product build (compiled without v_pk_*_f32, see csrc/fdcap.hip's build requirement); the Python
 * binding refuses a library that says otherwise unless FDCAP_ALLOW_PK_F32=1 (instrumentation variants). */
const char* fdcap_build_info(void);

/* Scene vertices, stored ONCE (the reference repeats them per frame, :175-176).  `scene_xyz`
 * is a HOST pointer [ns,3]; registered (copied, sorted into k-d cells and packed for the NN kernel -- on the device, one
 * synchronous call); ns <= FDCAP_MAX_SCENE_POINTS.
 * Both setters return FDCAP_E_STATE while an optimiser exists on the context (fdcap_opt_create .. fdcap_opt_destroy): its
 * buffers are sized for the registered sets and its pruning state (seeds, kept work lists) is only valid for them. */
int fdcap_set_scene(fdcap_ctx* ctx, const float* scene_xyz, int64_t ns);
/* Several registered scenes per context: slot 0 .. FDCAP_MAX_SCENES - 1, each with its own full table set, built exactly as
 * fdcap_set_scene builds its one (the same device build, the same FDCAP_SCENE_BUILD=host specification).  Slot 0 IS
 * fdcap_set_scene: fdcap_chamfer_fwd_scene / fdcap_chamfer_bwd_scene, ops.chamferDist's recognition of the registered scene,
 * fdcap_debug_scene_hash / fdcap_debug_scene_table and every optimiser but fdcap_opt_create_clips_scenes' mean slot 0.  For the
 * other slots ns = 0 clears the slot and frees its tables.  FDCAP_E_STATE while an optimiser exists (as fdcap_set_scene, for every
 * slot); FDCAP_E_ARG for a slot out of range. */
int fdcap_set_scene_slot(fdcap_ctx* ctx, int32_t slot, const float* scene_xyz, int64_t ns);
/* Diagnosis: out8[0..7] = FNV-1a hashes of the registered scene's device tables (input-order points, cell-ordered points, inverse
 * permutation, cell / quarter-cell / super-cell boxes, MFMA fragments, cell centres).  The tables are built on the device since r6
 * (csrc/fdc_scene.h); with FDCAP_SCENE_BUILD=host in the environment fdcap_set_scene takes the cell order from the host recursion of
 * r1-r5 instead -- the same order by specification.  Comparing the hashes of the two builds pins the ORDER only: both run the same
 * kernels for the boxes, fragments and centres.  Synchronises the device. */
int fdcap_debug_scene_hash(fdcap_ctx* ctx, uint64_t* out8);
/* Diagnosis: table `which` (0..7, the order of fdcap_debug_scene_hash) of the registered scene copied as it is to the HOST buffer
 * host_out, exactly *bytes bytes; host_out == NULL: *bytes <- the table's size.  FDCAP_E_ARG on a bad `which` or a size mismatch,
 * FDCAP_E_STATE without a registered scene.  Tests compare all eight tables byte for byte with an independent specification
 * (tests/scene_spec.py).  Synchronises the device. */
int fdcap_debug_scene_table(fdcap_ctx* ctx, int32_t which, void* host_out, int64_t* bytes);
/* Diagnosis: names of the kernel FORMS launched by this process since the last reset, "a;b;c" (several stages pick among forms by
 * row count and set size: blend products, contact forward, skinning backward, the Chamfer search).  Tests that mean to cover a form
 * check that it ran.  FDCAP_CLIP_FORMS_MIN_ROWS (environment, read once per process) lowers the row count from which the
 * clip-sized forms are selected (default 336): the reference's 300-frame fixtures then run through them. */
int fdcap_debug_kernel_forms(char* buf, int32_t len, int32_t reset);
/* test / diagnosis: one wave of the packed wave sums the skinning backward reduces with (csrc/fdc_math.h wave_sum64_pack) on the HOST
 * array in_h [64][n] (lane-major), 1 <= n <= 16: packed_h [n] <- the packed tree's sums as its lanes hold them, each_h [n] <- the
 * one-value tree (wave_sum64) per value.  The two must agree bit for bit.  Synchronises the device. */
int fdcap_debug_wave_sum_pack(const float* in_h, int32_t n, float* packed_h, float* each_h);
/* test / diagnosis: what the library holds in this process right now, out3 = {live memory blocks (device and pinned host), their
 * bytes, live HIP events}.  Every allocation and every event of the library is owned by a type of csrc/fdc_own.h that counts here
 * where it allocates and frees; nothing on a per-iteration path does.  A create ... destroy pair leaves all three where they were
 * (tests/test_gpu_ownership.py takes such differences). */
int fdcap_debug_live_allocations(int64_t out3[3]);
/* test / diagnosis: the joint sets of the optimiser's last pose forward and pose backward launch,
   out8 = {forward jn, jr, nlev, world; backward jn, jr, nlev, world}: joints [0, jn) took part in the kinematic chain,
   joints [0, jr) had their local rotation formed, nlev levels of the tree were walked, world = the world joints were written */
int fdcap_debug_pose_joint_sets(fdcap_ctx* c, int32_t* out8);
/* Contact vertex ids = get_contact_id(...) (global_optimization.py:79-94, :288); HOST pointer. */
int fdcap_set_contact_ids(fdcap_ctx* ctx, const int64_t* vid, int32_t nc);

/* ---- Op 1: Chamfer (ext.chamferDist()(xyz1, xyz2), global_optimization.py:292-294) -------- */
/* xyz1_d [B,n,3] queries, xyz2_d [B,m,3] targets with batch stride `stride2` elements
 * (0 = one scene shared by all batches).  Writes dist1_d [B,n] (squared L2 to the nearest
 * target, direct-difference form) and idx1_d [B,n] (lowest index among ties).  If dist2_d is
 * non-null also the reverse direction dist2_d [B,m], idx2_d [B,m] (the reference discards it).
 * Per-batch targets and the reverse direction run as one launch set over all batches (the batch on the grid's y axis);
 * FDCAP_CHAMFER_BATCHED=0, read on every call, runs them batch by batch instead -- the same bits. */
int fdcap_chamfer_fwd(fdcap_ctx* ctx, const float* xyz1_d, const float* xyz2_d, int32_t B,
                      int32_t n, int32_t m, int64_t stride2, float* dist1_d, int32_t* idx1_d,
                      float* dist2_d, int32_t* idx2_d, void* stream);
/* The same operator when xyz2 IS the scene registered with fdcap_set_scene -- the call site :292-294 passes the one scene in every
 * iteration of the caller's loop.  dist1_d / idx1_d [B,n] as fdcap_chamfer_fwd writes them, bit for bit (idx: original scene
 * indices, lowest among ties), found by the optimiser loop's search instead of visiting every pair: k-d-sorted scene, cell boxes,
 * seeds from the previous call's neighbours while B * n stays the same (first call / forget != 0: cheap fresh seeds), kept work
 * lists.  Library-owned state, one per context: calls on one context are serialised by the caller as everywhere.  FDCAP_E_STATE
 * without a registered scene.  fdcap_chamfer_bwd_scene: the matching gradient wrt the queries (fdcap_chamfer_bwd's formula, the
 * scene points read from the library's copy).  fdcap_chamfer_fwd itself accepts dist1_d == NULL (only the reverse direction). */
int fdcap_chamfer_fwd_scene(fdcap_ctx* ctx, const float* xyz1_d, int32_t B, int32_t n, float* dist1_d, int32_t* idx1_d, int32_t forget,
                            void* stream);
int fdcap_chamfer_bwd_scene(fdcap_ctx* ctx, const float* xyz1_d, int32_t B, int32_t n, const float* gdist1_d, const int32_t* idx1_d,
                            float* gxyz1_d, void* stream);
/* The dist1 half's gradient wrt the queries alone, the hot path of a loop that does not differentiate through its target:
 * gxyz1_d[b,i] = 2 g1[b,i] (x1[b,i]-x2[b,idx]).  The target's gradient and the dist2 half: fdcap_chamfer_bwd_both. */
int fdcap_chamfer_bwd(fdcap_ctx* ctx, const float* xyz1_d, const float* xyz2_d, int32_t B,
                      int32_t n, int32_t m, int64_t stride2, const float* gdist1_d,
                      const int32_t* idx1_d, float* gxyz1_d, void* stream);
/* The whole backward: both halves, both inputs, computed by the library in a defined order (no float atomics: the same bits in
 * every run, whatever the launch geometry; O(1) launches in B).  Every operation is fp32 and rounded on its own:
 *   a[b,i,k] = (2 g1[b,i]) (x1[b,i,k] - x2[b,j,k]), j = idx1[b,i]          (+0 without the dist1 term)
 *   u[b,j,k] = (2 g2[b,j]) (x2[b,j,k] - x1[b,i,k]), i = idx2[b,j]          (+0 without the dist2 term)
 *   gxyz1[b,i,k] = a[b,i,k] - S1,  S1 = +0, then + u[b,j,k] for every j with idx2[b,j] == i, ascending j
 *   gxyz2[b,j,k] = u[b,j,k] - S2,  S2 = +0, then + a[b,i,k] for every i with idx1[b,i] == j, ascending i
 *   reduce2 != 0 (one shared target, stride2 == 0): gxyz2[j,k] = U - A,  U = +0, then + u[b,j,k] ascending b;
 *                                                   A = +0, then + a[b,i,k] for every (b,i) with idx1[b,i] == j, ascending (b,i)
 * An index outside its range (-1: "no neighbour") makes its term +0 everywhere and is never used as an address.
 * gdist1_d / idx1_d [B,n]: both NULL = no dist1 term; gdist2_d / idx2_d [B,m]: both NULL = no dist2 term.  gxyz1_d [B,n,3] or
 * NULL; gxyz2_d NULL, [B,m,3] (reduce2 == 0) or [m,3] (reduce2 != 0).  FDCAP_E_ARG: a null ctx / xyz1_d / xyz2_d, a size <= 0,
 * a gradient without its indices or the reverse, no term or no output at all, reduce2 with stride2 != 0, B*n or B*m above
 * 2^31 - 1 (a side whose terms have to be grouped: above 2^31 - 8193).  Workspace: context-owned sort scratch, 16 bytes per
 * grouped term of the larger side, grown on demand and kept. */
int fdcap_chamfer_bwd_both(fdcap_ctx* ctx, const float* xyz1_d, const float* xyz2_d, int32_t B, int32_t n, int32_t m, int64_t stride2,
                           const float* gdist1_d, const int32_t* idx1_d, const float* gdist2_d, const int32_t* idx2_d,
                           float* gxyz1_d, float* gxyz2_d, int32_t reduce2, void* stream);

/* ---- Op 4: self-interpenetration of the body mesh (csrc/fdc_collide.h states the set, the order and the penalty in full) ---- */
/* Registers the mesh whose faces are tested against each other, static per context like the contact set: faces [n_faces,3] vertex
 * indices; face_part [n_faces] in 0..63 (NULL: all 0); ignore [64], a 64 x 64 bit matrix (NULL: none): bit (part[s], part[t]) or bit
 * (part[t], part[s]) drops the pair {s, t}.  The faces are ordered once, by the template's face centroids, under a box tree whose shape
 * never changes (leaves of 32 faces; FDCAP_COLL_LEAF=64, or a mesh above 32 768 faces: of 64).  Also readies the full-mesh vertex set.
 * n_faces = 0 clears the mesh.  FDCAP_E_ARG: n_faces outside {0} and [3, 65535], a vertex index outside [0, V), a part above 63.
 * FDCAP_E_STATE: a live optimiser (as scene registration). */
int fdcap_set_collision_mesh(fdcap_ctx* ctx, int32_t n_faces, const int32_t* faces, const uint8_t* face_part, const uint64_t* ignore);
typedef struct {
    float sigma;        /* the cone's opening, in (0, 1) */
    float w_coll;       /* weight of the term (not squared), finite and >= 0 */
    int32_t capacity;   /* pairs kept per frame, > 0 */
    int32_t every_pair; /* != 0: every pair of faces is tested, no tree (the checker: the same pairs, loss and gradient bit for bit) */
} fdcap_collision_params;
/* verts_d [n,V,3] world vertices -> per frame the pairs of faces that intersect and the penalty on them:
 *   count_d [n]              pairs FOUND (above capacity: the frame's list overflowed and holds the first `capacity` in list order)
 *   pairs_d [n,capacity,2]   or NULL: face ids as registered, the face earlier in tree order first, the list ordered by tree
 *                            position (owner, then other); -1 behind the kept pairs
 *   loss_d [n]               w_coll x (the kept pairs' values added in list order)
 *   dverts_d [n,V,3]         or NULL: d loss / d verts, the total derivative (the receiving face's normal, circumcentre and radius
 *                            move with its corners); per vertex its contributions added in ascending (list position, corner) order
 * No float atomics: the same call gives the same bits.  A face with a non-finite corner or |e0 x e1|^2 <= 1e-30 is in no pair.
 * Keeps no state between calls beyond workspace (context-owned, grown on demand: 4 bytes per face and frame, about 200 bytes per kept-pair slot
 * with dverts_d).  FDCAP_E_ARG: a null ctx / verts_d / params / count_d / loss_d, n <= 0, sigma outside (0, 1), a negative or
 * non-finite weight, capacity <= 0, 6 n capacity above 2^31 - 8193 or n V above 2^32 - 2.  FDCAP_E_STATE: no registered mesh. */
int fdcap_collision_eval(fdcap_ctx* ctx, const float* verts_d, int32_t n, const fdcap_collision_params* params, int32_t* pairs_d,
                         int32_t* count_d, float* loss_d, float* dverts_d, void* stream);
/* test / diagnosis: the registered mesh's tree.  info4 = {faces, leaf size, leaves, leaves padded to a power of two}; order_out (may
 * be NULL) [leaves x leaf size]: tree position -> face id, -1 behind the last face.  FDCAP_E_STATE: no registered mesh. */
int fdcap_debug_collision_tree(fdcap_ctx* ctx, int32_t* info4, int32_t* order_out);
/* test / diagnosis: the tree's boxes refit to verts_d [n,V,3], the refit kernel alone.  nodes_out_d (DEVICE) [n][2 x padded leaves][6]:
 * node i's {lo x y z, hi x y z} in heap numbering (root 1, leaf l = padded leaves + l); an empty node is {+inf, -inf}; node 0 is
 * unspecified.  FDCAP_E_ARG: a null ctx / verts_d / nodes_out_d, n <= 0.  FDCAP_E_STATE: no registered mesh. */
int fdcap_debug_collision_nodes(fdcap_ctx* ctx, const float* verts_d, int32_t n, float* nodes_out_d, void* stream);

/* Nearest-neighbour kernel selection for A/B measurement: 0 = by size (default), 1 = plain VALU
 * scan (nn_direct_kernel), 2 = MFMA-filtered exact scan (nn_mfma_kernel).  Both give bit-identical
 * results.  Process-wide. */
int fdcap_set_nn_kernel(int32_t mode);

/* ---- Op 3: VPoser decode (self.vposer.decode(z,'aa'), global_optimization.py:270-271) ----- */
/* z_d [B,32] with row stride ldz -> rot_d [B,21,9] rotation matrices; aa_d (optional) [B,63]. */
int fdcap_vposer_decode(fdcap_ctx* ctx, const float* z_d, int32_t ldz, int32_t B, float* rot_d,
                        float* aa_d, void* stream);
/* Its backward -- what loss.backward() (:591) runs through the reference's vposer.decode: gradients of the rotation
 * matrices g_rot_d [B,21,9] and / or of the angle-axis output g_aa_d [B,63] (either may be NULL, not both; the aa path
 * goes through torchgeometry's rotation_matrix_to_angle_axis, cvae.py:83) -> g_z_d [B,32].  The operator keeps no
 * state: the decoder's activations are recomputed from z_d. */
int fdcap_vposer_decode_bwd(fdcap_ctx* ctx, const float* z_d, int32_t ldz, int32_t B, const float* g_rot_d,
                            const float* g_aa_d, float* g_z_d, void* stream);

/* ---- Op 2: body model (self.body_mesh_model(...), global_optimization.py:280-283) ---------- */
/* params_d [B,75] file layout rows (transl, global_orient aa, betas, latent, lh, rh, cam_t);
 * runs VPoser + SMPL-X and writes vertices_d [B,V,3] and joints_d [B,55,3] (either optional),
 * body frame, `+transl` applied, no scale / world transform. */
int fdcap_body_forward(fdcap_ctx* ctx, const float* params_d, int32_t B, float* vertices_d,
                       float* joints_d, void* stream);
/* World-space mesh of saved results, as global_vis.py:126-152 builds it per frame on the CPU:
 * vertices_d [B,V,3] = camera_ext_b @ T(cam_t_b * scale) applied to scale * (SMPL-X(VPoser(row_b)) + transl).
 * params_d [B,75] rows as saved (:633), cam_ext_d [B,16], scale_d [1] device scalar. */
int fdcap_world_mesh(fdcap_ctx* ctx, const float* params_d, int32_t B, const float* cam_ext_d,
                     const float* scale_d, float* vertices_d, void* stream);
/* The same with the operator's own argument list (:280-283): global_orient_d [B,3] and
 * body_pose_d [B,63] axis-angle (Rodrigues as smplx.lbs.batch_rodrigues), betas_d [B,10],
 * left/right_hand_pose_d [B,12] PCA coefficients, transl_d [B,3]. */
int fdcap_smplx_forward(fdcap_ctx* ctx, const float* global_orient_d, const float* body_pose_d,
                        const float* betas_d, const float* left_hand_pose_d,
                        const float* right_hand_pose_d, const float* transl_d, int32_t B,
                        float* vertices_d, float* joints_d, void* stream);
/* Its backward (loss.backward() through self.body_mesh_model(...), :280-283 / :591): gradients of the outputs
 * g_vertices_d [B,V,3] and / or g_joints_d [B,55,3] (either may be NULL, not both) -> gradients of the six inputs (any
 * may be NULL).  Same inputs as the forward; its state is recomputed.  LBS, the K = 3V blend-shape data gradient, the
 * reverse kinematic chain and Rodrigues' backward are the kernels of mode 'local''s full-mesh backward. */
int fdcap_smplx_backward(fdcap_ctx* ctx, const float* global_orient_d, const float* body_pose_d,
                         const float* betas_d, const float* left_hand_pose_d,
                         const float* right_hand_pose_d, const float* transl_d, int32_t B,
                         const float* g_vertices_d, const float* g_joints_d, float* g_global_orient_d,
                         float* g_body_pose_d, float* g_betas_d, float* g_left_hand_pose_d,
                         float* g_right_hand_pose_d, float* g_transl_d, void* stream);
/* Op 2 WITH THE FITTED FACE (csrc/fdc_face_mesh.h): the four entry points above with the two keys the inner fit writes next to its
 * rows -- jaw_pose_d [B,3], joint 22's axis-angle (the same Rodrigues as the fit's jaw), and expression_d [B,10], SMPL-X's expression
 * coefficients (shapedirs' columns 10..19).  Each may be NULL on its own (the jaw shut, psi = 0); with both NULL a call is the entry
 * point without `_face`: the same launches, the same bits.  Vertices and the 55 joints are those of smplx with `expression` in the
 * shape components and `jaw_pose` in joint 22's slot (the jaw moves no joint).  The backward adds g_jaw_pose_d [B,3] and
 * g_expression_d [B,10] (NULL: not wanted; FDCAP_E_ARG for the gradient of an input that is NULL); every sum runs in a fixed order, so
 * two calls give the same bits.
 * FDCAP_E_STATE: expression_d on a model with num_shape < 20.  FDCAP_E_ARG: jaw_pose_d on a model whose joint 22 has a child. */
int fdcap_body_forward_face(fdcap_ctx* ctx, const float* params_d, int32_t B, const float* jaw_pose_d, const float* expression_d,
                            float* vertices_d, float* joints_d, void* stream);
int fdcap_world_mesh_face(fdcap_ctx* ctx, const float* params_d, int32_t B, const float* jaw_pose_d, const float* expression_d,
                          const float* cam_ext_d, const float* scale_d, float* vertices_d, void* stream);
int fdcap_smplx_forward_face(fdcap_ctx* ctx, const float* global_orient_d, const float* body_pose_d, const float* betas_d,
                             const float* left_hand_pose_d, const float* right_hand_pose_d, const float* transl_d, int32_t B,
                             const float* jaw_pose_d, const float* expression_d, float* vertices_d, float* joints_d, void* stream);
int fdcap_smplx_backward_face(fdcap_ctx* ctx, const float* global_orient_d, const float* body_pose_d, const float* betas_d,
                              const float* left_hand_pose_d, const float* right_hand_pose_d, const float* transl_d, int32_t B,
                              const float* jaw_pose_d, const float* expression_d, const float* g_vertices_d, const float* g_joints_d,
                              float* g_global_orient_d, float* g_body_pose_d, float* g_betas_d, float* g_left_hand_pose_d,
                              float* g_right_hand_pose_d, float* g_transl_d, float* g_jaw_pose_d, float* g_expression_d, void* stream);

/* ---- parameter-vector conversions (global_optimization.py:96-115, cvae.py:62-93) ----------- */
int fdcap_params_75_to_78(const float* p75_d, int32_t B, float* x78_d, void* stream);
int fdcap_params_78_to_75(const float* x78_d, int32_t B, float* p75_d, void* stream);

/* ---- the optimiser loop (FittingOP.init + fitting('global'), :450-489, :558-593) ----------- */
/* Allocates scratch for n_local (+2 halo rows each side) frames and REGISTERS the caller-owned
 * optimiser state (kept alive by the caller until fdcap_opt_destroy; a multi-GPU caller hands the
 * same tensors to RCCL):
 *   rows_x_d   [n_local+4,78] body_rotation_rec (:180) with 2 halo rows each side; owned rows start at 2
 *   rows_cam_d [n_local+4,16] camera_ext (:182), same row layout
 *   scale_d    [1]  scale (:179); set to cfg->scale_init here
 *   dscale_d   [1]  this rank's d loss / d scale (sum over owned frames): written by fdcap_opt_step /
 *              fdcap_opt_step_rows_and_pack (fused with the update) and, when log_terms != 0, by the backward
 *   losses_d   [FDCAP_NUM_LOSSES] double: this rank's un-normalised partial sums of the last
 *              backward that ran with log_terms != 0 (other iterations do not form them):
 *              [0] sum|x0-x|*mask  [1] sum z^2  [2] sum|2nd diff|  [3] sum r/(r+1)
 *              [4] sum|Jw_i-Jw_{i+1}| */
int fdcap_opt_create(fdcap_ctx* ctx, const fdcap_opt_config* cfg, float* rows_x_d, float* rows_cam_d,
                     float* scale_d, float* dscale_d, double* losses_d);
/* A BATCH of n_clips clips of N frames each, fitted as one optimisation (fdcap_opt_create is the n_clips = 1 case of this call).
 * cfg: n_total == n_local == N (the clip length), frame0 == 0; the clips share the scene, the contact ids, the body model and
 * cfg.  Every clip keeps its own rows, `scale`, Adam moments (of all three), outlier mask, loss means (over its own N frames)
 * and logged sums; the temporal stencils are cut at clip boundaries, and all clips share the iteration counter.
 *   rows_x_d   [n_clips*N+4,78]  clip k owns rows 2 + k*N .. 2 + (k+1)*N (fdcap_opt_set_inputs takes the n_clips*N rows)
 *   rows_cam_d [n_clips*N+4,16]  same rows
 *   scale_d    [n_clips]          set to cfg->scale_init each;  dscale_d [n_clips]: each clip's d loss / d scale
 *   losses_d   [n_clips][FDCAP_NUM_LOSSES] double: each clip's partial sums
 * A clip's results equal its stand-alone fit (fdcap_opt_create with n_total = n_local = N) bit for bit when both select the same
 * kernel forms (chosen by row count: FDCAP_CLIP_FORMS_MIN_ROWS pins them); with the default forms only the rounding of the data
 * gradient's sum may differ.  The batch takes the single-GPU schedule (deferred row step, `scale` stepped by the backward's tail).
 * Calls that cover the optimiser's rows cover all n_clips*N of them (fdcap_opt_get_results, fdcap_opt_forward_world,
 * fdcap_opt_get_contact, fdcap_opt_get_grads, launch timing); fdcap_opt_get_results writes n_clips scales; the state of
 * fdcap_opt_export_state holds n_clips scale moments; fdcap_opt_run's history rows are [n_clips][FDCAP_NUM_LOSSES].
 * Modes: 'global'; 'local' -- its first loop is fdcap_opt_run under the 'local' config (phase1_contact = 0.2, phase2_world = 0),
 * its second loop fdcap_opt_run_local2, the ONE call through which a batch reaches detect_contact and cal_loss2; and 'dct' --
 * fdcap_opt_set_dct_clips, then fdcap_opt_run_dct, the ONE call through which a batch reaches both of that mode's phases.  With
 * n_clips > 1 these return FDCAP_E_STATE: mode 'local''s single steps (fdcap_opt_detect_contact, fdcap_opt_backward_local2), mode
 * 'dct''s (fdcap_opt_set_dct, fdcap_opt_dct_fit, fdcap_opt_backward_dct; its read-backs fdcap_opt_get_dct .. fdcap_opt_set_dct_state
 * until fdcap_opt_set_dct_clips has run), the per-frame inner fit (fdcap_opt_set_keypoints, fdcap_opt_backward_fit2d,
 * fdcap_opt_step_x, fdcap_opt_fit2d_lbfgs[_stats]), fdcap_opt_forward_ahead and the exchange calls (fdcap_opt_step_rows_and_pack,
 * fdcap_opt_unpack_and_step_scale, fdcap_opt_halo_exchange, fdcap_opt_exchange, fdcap_opt_time_exchange, fdcap_opt_run with
 * flags bit 1).  FDCAP_E_ARG: n_clips < 1, or n_clips > 1 with frame0 != 0 or n_local != n_total. */
int fdcap_opt_create_clips(fdcap_ctx* ctx, const fdcap_opt_config* cfg, int32_t n_clips, float* rows_x_d, float* rows_cam_d,
                           float* scale_d, float* dscale_d, double* losses_d);
/* The same batch with clips of their OWN lengths clip_len[0 .. n_clips) (host array, copied): clip k owns rows 2 + s_k .. 2 + s_k +
 * clip_len[k], s_k = clip_len[0] + .. + clip_len[k-1].  cfg: frame0 == 0 and n_total == n_local == the sum of the lengths; the
 * buffers are [sum + 4, .] rows, scale_d / dscale_d / losses_d per clip as above.  Same contract: every clip's means run over its
 * own frame count, its stencils end at its own first and last frame, and its results equal its stand-alone fit bit for bit when
 * both select the same kernel forms (a clip of one or two frames has no smoothing term, of one frame no world-smoothing term, as in
 * a stand-alone fit).  Everything above that covers "n_clips*N rows" covers the sum; the state of fdcap_opt_export_state is
 * [m_x sum*78 | v_x | m_cam sum*16 | v_cam | m_scale n_clips | v_scale n_clips].  Everything fdcap_opt_create_clips refuses with
 * n_clips > 1 is refused the same way.  Equal lengths ARE fdcap_opt_create_clips' batch (same kernels' arithmetic on the one
 * length, same bits); with different lengths the per-frame kernels read each frame's clip, index, length and normalised weights
 * from a small device table built here from cfg (csrc/fdc_clips.h).
 * FDCAP_E_ARG: clip_len NULL, a length <= 0, a sum that is not cfg->n_total == cfg->n_local or exceeds 2^24, frame0 != 0. */
int fdcap_opt_create_clips_var(fdcap_ctx* ctx, const fdcap_opt_config* cfg, int32_t n_clips, const int32_t* clip_len, float* rows_x_d,
                               float* rows_cam_d, float* scale_d, float* dscale_d, double* losses_d);
/* Clips of DIFFERENT SCENES in one batch: fdcap_opt_create_clips_var plus clip_scene [n_clips], the scene slot
 * (fdcap_set_scene_slot) clip k is fitted against.  A SEGMENT is a maximal run of adjacent clips of one slot (slots A, B, A: three
 * segments).  Only the Chamfer search knows segments: each searches its own scene with its own pruning state (kept lists, launch
 * and query order with their 32-launch cadence, seeding) -- one launch for all segments where the largest is large enough for the
 * one-wave streaming form, else (and with FDCAP_NN_SEGMENTS=loop in the environment at create) one launch set per segment; the
 * same bits either way.  Every other kernel sees the rows of fdcap_opt_create_clips_var's batch.  A clip's results equal its
 * stand-alone fit against its own scene bit for bit under equal kernel forms.
 * All clips on one slot: exactly fdcap_opt_create_clips_var (one segment, its path and bits), on that slot's scene.
 * Mode 'global' only: with more than one segment fdcap_opt_run_local2, fdcap_opt_set_dct_clips, fdcap_opt_run_dct,
 * fdcap_opt_time_chamfer(brute_force) and fdcap_debug_nn_query_order return FDCAP_E_STATE, on top of everything a batch is refused
 * (mode 'local''s and 'dct''s single steps, the per-frame inner fit, every exchange call, fdcap_opt_forward_ahead).
 * FDCAP_E_ARG: what fdcap_opt_create_clips_var refuses, clip_scene NULL or a slot outside [0, FDCAP_MAX_SCENES).  FDCAP_E_STATE:
 * a named slot holds no scene. */
int fdcap_opt_create_clips_scenes(fdcap_ctx* ctx, const fdcap_opt_config* cfg, int32_t n_clips, const int32_t* clip_len, const int32_t* clip_scene,
                                  float* rows_x_d, float* rows_cam_d, float* scale_d, float* dscale_d, double* losses_d);
/* data78_d [n_local,78]: the 6D-converted SMPLify-X rows (loss_rec target);
 * init78_d [n_local,78]: initial value of body_rotation_rec (= data with outlier rows replaced, :487);
 * mask_d   [n_local]   : 0 for outlier rows (idx1), 1 otherwise (:255-257);
 * cam_ext_d[n_local,16]: extract_ext() (:455).  All copied. */
int fdcap_opt_set_inputs(fdcap_ctx* ctx, const float* data78_d, const float* init78_d,
                         const float* mask_d, const float* cam_ext_d, void* stream);
/* The clip-level fit's 2D-keypoint reprojection term on the body joints (not in the reference, which has no such term: parity-unpinned
 * like the per-frame inner fit, and checked against an fp64 autograd twin of the definition instead, tests/reproj_spec.py).  Per frame
 * i of the clip's N = n_total frames and SMPL-X joint j in 0..22:
 *     p_ij = G_ij.t + transl_i + cam_t_i        camera frame; cam_t = row columns 75:78, NOT multiplied by `scale`
 *     u, v = fx p.x / p.z + cx,  fy p.y / p.z + cy
 *     loss_reproj = weight / (23 N) * sum_ij conf_ij^2 [ GMoF_rho(k^u_ij - u) + GMoF_rho(k^v_ij - v) ]
 * the frame SMPLify-X fitted in (body and camera offset both times `scale` cancel in the projection).  The term depends on neither
 * `scale` nor camera_ext -- by construction: its gradient enters the pose backward as the gradient of the posed body-frame joints and
 * never meets the world matrix -- and reaches the rows alone: transl, the rotations and betas through the chain, cam_t by sum_j of
 * the joints' gradients.  A keypoint with conf == 0 is skipped (value and gradient exact zeros, whatever its coordinates hold, NaN
 * included) and still counts in 23 N.  Outlier frames are not masked.  The term joins both phase totals with coefficient 1.
 *   kp_d DEVICE [n_local,23,3] (u, v, conf) in SMPL-X joint order, this rank's own rows (fdcap_opt_set_keypoints' layout); copied.
 *   params NULL or weight == 0: off -- then every launch is the one it was, with the arguments it had.
 * On: fdcap_opt_backward, fdcap_opt_backward_and_step and fdcap_opt_run carry the term, on a whole clip and on one rank's share (no
 * neighbour row is read: the exchange is untouched); a logging backward leaves the un-normalised partial sum
 * sum conf^2 [GMoF + GMoF] in losses_d [FDCAP_LOSS_REPROJ]; the pose kernels keep joints 0..22 in every iteration.  The term rides in
 * the pose backward's launch (pose_bwd_reproj_kernel in pose_bwd_kernel's place): an iteration has no launch more, and
 * fdcap_opt_launch_timing books it on FDCAP_LT_POSE_BWD.
 * FDCAP_E_ARG: fx, fy or rho non-finite or not positive, cx or cy non-finite, weight non-finite or negative, kp_d NULL with a non-zero
 * weight.  FDCAP_E_STATE: no optimiser, a batch of clips, a DCT term set up.  A refused call leaves the term as it was.  While the
 * term is on, fdcap_opt_run_local2, fdcap_opt_backward_local2, fdcap_opt_step_x and the DCT calls (fdcap_opt_set_dct[_clips],
 * fdcap_opt_dct_fit, fdcap_opt_backward_dct, fdcap_opt_run_dct) return FDCAP_E_STATE.  Every fdcap_opt_create* switches it off:
 * keypoints are an input of a fit, not state (a resumed fit hands them over again). */
typedef struct fdcap_reproj_params { float fx, fy, cx, cy, rho, weight; } fdcap_reproj_params;
int fdcap_opt_set_reproj(fdcap_ctx* ctx, const fdcap_reproj_params* params, const float* kp_d, void* stream);
/* One pass of the loop body :562-592 for iteration `ii` of `num_iter`, split in two so a
 * multi-GPU caller can all-reduce the scalar `scale` gradient in between:
 *   backward: zero_grad + cal_loss + loss.backward()  -> gradients + loss partial sums
 *   step    : optimizer.step() (fused Adam over body_rotation_rec, scale, camera_ext)
 * `phase2` = (ii >= 0.8*num_iter) decides the loss total; the requires_grad toggling of
 * :564-568/:577-580 (effective one forward late) is reproduced from ii and first_phase2_iter.
 * log_terms != 0: also evaluate what the reference only prints (:573-575, :587-589) -- the loss partial
 * sums in losses_d, the contact term in phase 2 -- and leave dscale_d valid after the backward.
 * log_terms == 2: the same terms, but losses_d is complete only after the fdcap_opt_step / fdcap_opt_step_rows_and_pack call
 * that follows (the fixed-order reduction of the per-frame partial sums rides in that launch: one launch less per logged
 * iteration; dscale_d as on a non-logging iteration). */
int fdcap_opt_backward(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, int32_t log_terms,
                       void* stream);
int fdcap_opt_step(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, void* stream);
/* loss.backward() + optimizer.step() of iteration ii (:591-592) in ONE call and without a launch for the step (r4): `scale` is
 * stepped by one more workgroup of the backward's last launch, the rows of body_rotation_rec / camera_ext take their update in
 * the first two launches of the next backward, where they are read anyway -- same arithmetic, same bits as fdcap_opt_backward
 * followed by fdcap_opt_step.  Until then rows_x_d / rows_cam_d and their Adam moments hold the PRE-step values: every other entry
 * point of this group applies a still-pending update first (an ordinary Adam launch), and a caller that reads the registered
 * buffers itself calls fdcap_opt_sync before it does.  log_terms == 2 here: the printed sums are reduced by that same extra
 * workgroup (losses_d complete when this call's work is).  Sharded runs and mode 'dct' take the two-call path, silently. */
int fdcap_opt_backward_and_step(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, int32_t log_terms, void* stream);
int fdcap_opt_sync(fdcap_ctx* ctx, void* stream);
/* The loop :560-593 itself -- iterations [ii0, ii1) of a fit of num_iter iterations -- in ONE call (r4): the sequence of the calls
 * above that FittingOP.fitting issues (fdcap_opt_backward_and_step; the fit's last iteration as fdcap_opt_backward + fdcap_opt_step;
 * on a sharded context, which must hold a communicator, fdcap_opt_backward + fdcap_opt_exchange), so the same bits.  Logging
 * iterations (log_every > 0: ii % log_every == 0, and ii == num_iter - 1; the reference prints every iteration) leave their partial
 * sums in consecutive rows of hist_d [hist_rows][FDCAP_NUM_LOSSES] on the device ([hist_rows][n_clips][FDCAP_NUM_LOSSES] for a
 * batch of clips, fdcap_opt_create_clips), *n_logged of them, with no host sync; the output
 * registered before the call is registered again after it.  flags bit 0: every optimiser step as its own launch; bit 1: the
 * exchange tail although the context holds the whole clip (a communicator of one rank).  Returns when the
 * work is enqueued.  A caller with something to do between iterations (snapshots, checkpoints, a finite check) calls it per stretch. */
int fdcap_opt_run(fdcap_ctx* ctx, int32_t ii0, int32_t ii1, int32_t num_iter, int32_t first_phase2_iter, int32_t log_every,
                  double* hist_d, int32_t hist_rows, int32_t flags, int32_t* n_logged, void* stream);
/* Checkpoint / resume (the reference only ever writes its final result, :637-653).  The parameters live in the
 * caller's registered tensors; these move the rest of the optimiser state -- Adam's moments of the owned rows:
 * state_d [fdcap_opt_state_len()] floats = [m_x n_local*78 | v_x | m_cam n_local*16 | v_cam | m_scale | v_scale]
 * (a batch of K clips: n_local = K*N rows, and m_scale / v_scale hold K values each).
 * The step counters are functions of the iteration index the caller passes to fdcap_opt_step; seeds and kept work lists of
 * the Chamfer search are pruning state only (results never depend on them) and are not part of a checkpoint.  Mode 'dct''s
 * c_dct moments are not covered. */
int32_t fdcap_opt_state_len(fdcap_ctx* ctx);
int fdcap_opt_export_state(fdcap_ctx* ctx, float* state_d, void* stream);
int fdcap_opt_import_state(fdcap_ctx* ctx, const float* state_d, void* stream);
/* count_d [1] int32 <- number of non-finite values among the owned rows of body_rotation_rec / camera_ext and scale (every
 * clip's, for a batch)
 * (the reference wraps every iteration in torch.autograd.set_detect_anomaly(True), :561, at ~4x the host cost; this is
 * the opt-in equivalent: FittingOP.fitting(check_finite_every=k)). */
int fdcap_opt_check_finite(fdcap_ctx* ctx, int32_t* count_d, void* stream);
/* Redirect the loss partial sums of the following logging backwards to another [FDCAP_NUM_LOSSES] double buffer (e.g. the
 * next row of a device-side history, so that a caller logging every iteration -- as the reference prints every
 * iteration, :573-575 -- needs no copy and no host sync inside the loop).  Host-side only; nothing is launched. */
int fdcap_opt_set_loss_output(fdcap_ctx* ctx, double* losses_d);
/* ---- mode 'local' (:499-556).  Its first loop is fdcap_opt_backward / _step with
 * phase1_contact = 0.2 and phase2_world = 0 in the config (:511, :523); then: */
/* detect_contact (:315-365): weight_left_d [n_local] = left / (left + left) per frame, `left` = mean
 * squared NN distance of the first n_left contact ids (the L_Leg part) -- the reference's own formula,
 * identically 0.5 (NaN where the distance is 0). */
int fdcap_opt_detect_contact(fdcap_ctx* ctx, int32_t n_left, float* weight_left_d, void* stream);
/* zero_grad + cal_loss2 + backward (:368-447, :538-554): loss = vertex-space second-difference smoothing
 * over ALL mesh vertices + parameter smoothing + loss_rec + foot-skate term; only body_rotation_rec gets
 * a gradient.  contact_weight_d [n_total]: detect_contact's output for the WHOLE clip (all ranks).
 * losses_d afterwards: [0] rec, [2] parameter smoothing, [5] vertex smoothing, [6] foot-skate (already
 * normalised per part). */
int fdcap_opt_backward_local2(fdcap_ctx* ctx, const float* contact_weight_d, int32_t n_left, void* stream);
/* Adam on body_rotation_rec only, with its running step count `step` (continues after the first loop). */
int fdcap_opt_step_x(fdcap_ctx* ctx, int32_t step, void* stream);
/* detect_contact (:534) and iterations [jj0, jj1) of mode 'local''s second loop (:536-556) in ONE call, for one clip or a BATCH of
 * clips (fdcap_opt_create_clips[_var]); call it after the first loop (fdcap_opt_run under the 'local' config) of num_iter iterations.
 *   contact_weight_d [n_local]: one weight per owned frame, in buffer-row order across the whole batch.  jj0 == 0: the call first
 *     runs detect_contact (pose forward, contact forward, left / (left + left) per frame) and WRITES it; jj0 > 0: it is an input
 *     (a resumed loop; a caller's own weights).
 *   Iteration jj: the launches of fdcap_opt_backward_local2, then fdcap_opt_step_x with Adam step number num_iter + jj + 1 -- for
 *     one clip the same launches and the same bits as those two calls.  For a batch every launch takes its clip-aware form: each
 *     clip's means run over its OWN frame count (w_rec = weight_loss_rec / (n 78), 1 / ((n - 2) 78), 1 / ((n - 2) 3V), the
 *     foot-skate 1 / ((n - 1) npart 3); no second difference below three frames, no first difference below two), the stencils
 *     end at the clip's first and last frame (foot-skate pair (i, i + 1) uses w[i + 1] of the same clip), every row reads its own
 *     clip's `scale`, and the sums go to the clip's own losses[k][].  A clip's results equal its stand-alone mode-'local' fit bit
 *     for bit when both select the same kernel forms.  The full-mesh buffers hold [rows + 4, 3V] floats, three of them.
 *   Logging iterations (log_every > 0: jj % log_every == 0) leave their partial sums -- slots [0] rec, [1] z^2, [2] parameter
 *     smoothing, [5] vertex smoothing, [6] foot skate (normalised per part), as fdcap_opt_backward_local2 -- in consecutive rows of
 *     hist_d [hist_rows][n_clips][FDCAP_NUM_LOSSES] on the device, *n_logged of them, with no host sync (they are sums of
 *     per-workgroup partials added with atomics: equal to a stand-alone fit's to rounding, not bit for bit); the other iterations
 *     use the registered losses_d, which is registered again before the call returns.
 *   flags bit 0: the LAST iteration of the stretch is not stepped -- its gradients stay readable through fdcap_opt_get_grads.
 * FDCAP_E_ARG: n_left <= 0 or >= the contact count, jj0 < 0, jj1 < jj0, contact_weight_d NULL, a stretch with logging iterations
 * and hist_d NULL or fewer than that many hist_rows.  FDCAP_E_STATE: no optimiser, no contact set, a DCT term set up, or a
 * sharded context (n_local != n_total: the halo exchange between two iterations stays with the caller, who issues the single
 * steps).  Returns when the work is enqueued. */
int fdcap_opt_run_local2(fdcap_ctx* ctx, int32_t n_left, int32_t jj0, int32_t jj1, int32_t num_iter, int32_t log_every,
                         float* contact_weight_d, double* hist_d, int32_t hist_rows, int32_t flags, int32_t* n_logged, void* stream);

/* ---- mode 'dct' (global_optimization.py:595-630) ---------------------------------
 * cal_dctloss (:232-246) over W = n_total / T windows of T frames (reference: 5 x 60, :41-42) and the 23
 * world joints x 3 axes; c_dct [W,23,3,C] and its Adam moments are library-owned.
 * fdcap_opt_set_dct: dct_mtx HOST [T,C] (= load_dct_base(), :131-136; T <= 64, C <= 8), c_dct_d DEVICE
 * [W,23,3,C] initial coefficients (the reference draws them with torch.randn, :186).  After fdcap_opt_create. */
int fdcap_opt_set_dct(fdcap_ctx* ctx, const float* dct_mtx, int32_t T, int32_t C, const float* c_dct_d, void* stream);
/* The first phase of the loop (:601-613): body_rotation_rec / scale / camera_ext are frozen, loss =
 * weight * loss_dct (weight = 10, :607), so `iters` Adam iterations on c_dct (step counters step0+1 ...)
 * run in one launch against the fixed world-joint trajectories of the current state.  Only windows that
 * lie inside this rank's frames are fitted.  obj_hist_d (optional) [ceil(iters/log_stride), 69*(w1-w0)]:
 * each fitted trajectory's objective (sum over the window of e/(e+1)) before the update of iterations
 * 0, log_stride, 2*log_stride ...
 * weight = 0: every gradient is exactly zero, so c_dct coasts on its Adam moments -- what torch < 2's
 * zero_grad() (grads zeroed, not None) does to the frozen c_dct from iteration ceil(0.95 num_iter) on
 * (legacy_zero_grad = 1 callers issue one such iteration per loop iteration); no forward runs. */
int fdcap_opt_dct_fit(fdcap_ctx* ctx, int32_t iters, int32_t step0, float weight, float* obj_hist_d,
                      int32_t log_stride, void* stream);
/* The second phase (:614-626): zero_grad + cal_loss + backward of
 *   loss = w_dct * loss_dct + w_rec * loss_rec + w_contact * loss_contact   (1e-4, 0.5, 0.1 at :620);
 * body_rotation_rec and scale get gradients, c_dct / camera_ext do not.  Step with fdcap_opt_step(ctx, k,
 * INT32_MAX, ...) (k = 0, 1, ...: both Adam step counters start at 1 here) or the multi-GPU pair below.
 * losses_d afterwards: [0] [1] [3] as fdcap_opt_backward, [7] = un-normalised sum of e/(e+1) over this
 * rank's frames (loss_dct = sum / (69 W)). */
int fdcap_opt_backward_dct(fdcap_ctx* ctx, float w_dct, float w_rec, float w_contact, int32_t log_terms, void* stream);
/* c_dct_d [W,23,3,C] <- current coefficients (a sharded caller merges the windows each rank fitted);
 * fdcap_opt_set_dct_coef writes merged coefficients back without touching the Adam moments. */
int fdcap_opt_set_dct_coef(fdcap_ctx* ctx, const float* c_dct_d, void* stream);
int fdcap_opt_get_dct(fdcap_ctx* ctx, float* c_dct_d, void* stream);
/* Adam's two moments of c_dct, DEVICE [W,69,C] each (zero after fdcap_opt_set_dct): with fdcap_opt_get_dct and
 * fdcap_opt_export_state the whole optimiser state of mode 'dct' -- a fit continued from them (fdcap_opt_dct_fit with step0 = the
 * iterations already made) ends on the uninterrupted fit's bits. */
int fdcap_opt_get_dct_state(fdcap_ctx* ctx, float* m_d, float* v_d, void* stream);
int fdcap_opt_set_dct_state(fdcap_ctx* ctx, const float* m_d, const float* v_d, void* stream);
/* Returns W; *w0 / *w1 = first / one-past-last window this rank fits (0 when fdcap_opt_set_dct has not run).  A batch
 * (fdcap_opt_set_dct_clips): W = the windows of all clips, *w0 = 0, *w1 = W. */
int32_t fdcap_opt_dct_windows(fdcap_ctx* ctx, int32_t* w0, int32_t* w1);
/* Mode 'dct' for WHOLE clips: an optimiser of fdcap_opt_create_clips / fdcap_opt_create_clips_var, or one clip (then exactly
 * fdcap_opt_set_dct).  Clip k of n_k frames has W_k = n_k / T windows over its own frames [0, W_k T); its trailing n_k % T frames
 * belong to no window, as in a stand-alone fit.  dct_mtx HOST [T,C]; c_dct_d DEVICE [sum W_k, 23, 3, C], clip after clip (copied; the
 * Adam moments are library-owned and zeroed).  Afterwards fdcap_opt_get_dct, fdcap_opt_set_dct_coef and fdcap_opt_get/set_dct_state
 * serve the batch with arrays of that layout, and the loop runs through fdcap_opt_run_dct.  Every clip's mean runs over its own
 * 69 W_k trajectories and lands on the bits of its stand-alone fit under equal kernel forms.
 * FDCAP_E_ARG: a clip with W_k = 0 (the stand-alone fit refuses it too), T > 64, C > 8.  FDCAP_E_STATE: no optimiser, or one that
 * holds a shard of a clip (n_local != n_total). */
int fdcap_opt_set_dct_clips(fdcap_ctx* ctx, const float* dct_mtx, int32_t T, int32_t C, const float* c_dct_d, void* stream);
/* starts HOST [n_clips + 1] <- each clip's first window in c_dct (starts[n_clips] = fdcap_opt_dct_windows' W); n = n_clips + 1.
 * FDCAP_E_STATE without a DCT term. */
int fdcap_opt_dct_clip_windows(fdcap_ctx* ctx, int32_t* starts, int32_t n);
/* Iterations [ii0, ii1) of mode 'dct''s loop of a fit of num_iter in ONE call (one clip or a batch, after fdcap_opt_set_dct_clips),
 * P = ceil(0.95 num_iter):
 *   ii < P   the first phase, ONE fdcap_opt_dct_fit launch over every clip's trajectories with weight w_phase1 (10 at :607); the
 *            step counters run on from ii0, so a stretch cut anywhere gives the one-call bits.  obj_hist_d (optional; used when
 *            log_every > 0) DEVICE [ceil((min(ii1, P) - ii0) / log_every)][69 W] as fdcap_opt_dct_fit writes it;
 *   ii == P  nothing is stepped (cfg.legacy_zero_grad: c_dct coasts one step);
 *   ii > P   fdcap_opt_backward_dct(w_dct, w_rec, w_contact) + fdcap_opt_step(ii - P - 1, 2^30): the rows and each clip's scale with
 *            step number ii - P (cfg.legacy_zero_grad: a coasting fdcap_opt_dct_fit(weight 0) follows each step).
 * Second-phase logging iterations (log_every > 0: ii % log_every == 0, and ii == num_iter - 1) write their per-clip partial sums
 * (slots 0, 1, 2, 3, 7) to consecutive rows of hist_d DEVICE [hist_rows][n_clips][FDCAP_NUM_LOSSES], without a host sync;
 * *n_logged rows used.  flags bit 0: the stretch's last iteration is left unstepped for fdcap_opt_get_grads.  Clips of different
 * lengths take their per-frame weights from records built by fdcap_opt_set_dct_clips under w_rec = 0.5, w_contact = 0.1 (:620):
 * other values there are FDCAP_E_STATE (w_dct is free).  Nothing here waits for the device.
 * FDCAP_E_ARG: ii0 < 0, ii1 < ii0, ii1 > num_iter, log_every < 0, a second-phase logging iteration in the stretch with hist_d NULL
 * or fewer than that many hist_rows.  FDCAP_E_STATE: no optimiser, no DCT term, a shard of a clip. */
int fdcap_opt_run_dct(fdcap_ctx* ctx, int32_t ii0, int32_t ii1, int32_t num_iter, float w_phase1, float w_dct, float w_rec,
                      float w_contact, int32_t log_every, float* obj_hist_d, double* hist_d, int32_t hist_rows, int32_t flags,
                      int32_t* n_logged_out, void* stream);

/* ---- optimization.py: the per-frame smoother (:185-238, driver loop :334-348) -------
 * data78_d [N,78] = convert_to_6D_rot of the SMPLify-X rows in file order; for every frame `iters` (50, :313)
 * Adam iterations (lr 0.1, :312) on one 78-d row started at the data row, with
 *   loss = w_rec * L1(data, x) + w_vposer * mean(x[19:51]^2) [+ w_prev * L1(previous result[9:51], x[9:51])]
 * (1, 0.001, 5: :197, :227, :323-324); frame 0 has no previous-frame term (:185-208).  torch's optimiser
 * object is created once (:126), so Adam's moments and step counter carry over from frame to frame -- kept.
 * out78_d [N,78]: the optimised rows (fdcap_params_78_to_75 gives the saved layout, :206, :236).
 * state_d (optional) DEVICE [3,78] = Adam m | v | previous frame's result: read when step0 > 0 or has_prev,
 * always written, so a caller can go file by file like the reference's driver; step0 = Adam steps taken so
 * far (frames done x iters), has_prev = the first row of this call has a predecessor.  `ctx` only lends a
 * workspace and may be NULL (the body model plays no part, although the reference loads it, :106-123); the
 * call then synchronises `stream` before it returns. */
int fdcap_frame_smoother(fdcap_ctx* ctx, const float* data78_d, int32_t N, int32_t iters, float lr, float w_rec,
                         float w_vposer, float w_prev, float* state_d, int32_t step0, int32_t has_prev,
                         float* out78_d, void* stream);

/* ---- per-frame inner fit with a true 2D-keypoint reprojection residual (BASELINE config 4) ----
 * NOT part of the reference repository: there the per-frame fit is the external SMPLify-X step (README.md:14-17) and
 * the only in-repo projection is a viewer overlay (local_vis.py:368-378; intrinsics fx = fy = 692, cx = 640, cy = 360,
 * vis.py:358-360).  Objective restated from the published SMPLify-X data term and L2 priors (csrc/fdc_fit2d.h);
 * frames are independent.  Use: fdcap_opt_create (scale_init = 1), fdcap_opt_set_inputs (camera_ext rows = identity, so
 * the "world" joints are camera-frame joints + camera_translation), fdcap_opt_set_keypoints, then per iteration
 * fdcap_opt_backward_fit2d + fdcap_opt_step_x; fdcap_opt_reset_adam between stages; fdcap_opt_get_results.
 * The evaluation itself honours whatever camera_ext rows and scale the registered buffers hold -- points are projected from the
 * clip-level loop's world frame, and fdcap_opt_get_grads' d camera_ext is that evaluation's (tests/test_gpu_world_frame.py) -- while
 * the start from keypoints alone (fdcap_opt_fit2d_guess, the camera stage, fdcap_fit2d_flip_orient, fdcap_fit2d_select;
 * csrc/fdc_fit2d_init.h) is written for the identity set-up and does not. */
typedef struct fdcap_fit2d_stage {
    float fx, fy, cx, cy;   /* pinhole intrinsics */
    float rho;              /* GMoF scale in pixels (SMPLify-X: 100) */
    float w_data, w_pose, w_shape, w_hand;   /* stage weights (enter squared) */
} fdcap_fit2d_stage;
/* kp_d DEVICE [n_local,23,3]: (u, v, confidence) of SMPL-X joints 0..22 (the joints[:, 0:23] the reference reads, :298). */
int fdcap_opt_set_keypoints(fdcap_ctx* ctx, const float* kp_d, void* stream);
/* ... on a detector's keypoints (csrc/fdc_keypoints.h): a map, static per context, from keypoint k to an SMPL-X joint or a point of
 * the mesh surface.  Every kind's position is "SMPL-X output + transl + camera_translation" under the inner fit's set-up above
 * (camera_ext rows = identity, scale = 1); joints 0..22 are the 23-joint path's own world joints, so a map of exactly those in
 * order gives that path's bits.  At scale != 1 the finger joints 23..54 follow the vertex formula, camera_ext R [scale (p + transl +
 * camera_translation)] + t (the kernel forms them as pseudo-vertices), and not the world joints' R [(J + transl) + scale
 * camera_translation] + t. */
#define FDCAP_MAX_KEYPOINTS 160
/* joint[k] >= 0: SMPL-X joint; joint[k] < 0: surface point tri[k][0..2] (vertex ids), bary[k][0..2].  HOST arrays.
 * n_kp = 0 clears the map.  FDCAP_E_ARG: n_kp < 0 or > FDCAP_MAX_KEYPOINTS, joint >= 55, a vertex id outside [0, V),
 * a non-finite weight.  FDCAP_E_STATE: a live optimiser (as scene registration). */
int fdcap_set_keypoint_map(fdcap_ctx* ctx, int32_t n_kp, const int32_t* joint, const int32_t* tri, const float* bary);
/* kp_d DEVICE [n_local, n_kp, 3] (u, v, confidence) in map order.  From here on fdcap_opt_backward_fit2d,
 * fdcap_opt_fit2d_lbfgs and its stats use the mapped data term; fdcap_opt_set_keypoints switches back.
 * FDCAP_E_STATE without a map or for a batch of clips (as fdcap_opt_set_keypoints). */
int fdcap_opt_set_keypoints_mapped(fdcap_ctx* ctx, const float* kp_d, void* stream);
/* the mapped keypoints' camera-frame 3D positions of the current rows, out_d DEVICE [n_local, n_kp, 3] (diagnostic; runs the forward) */
int fdcap_debug_keypoints3d(fdcap_ctx* ctx, float* out_d, void* stream);
/* zero_grad + loss + backward; only body_rotation_rec gets a gradient.  log_terms != 0: losses_d [0] = data term,
 * [1] = priors (both already weighted, summed over this rank's frames).  (The latent columns' gradient is left in the VPoser
 * backward's four partial arrays; fdcap_opt_step_x and fdcap_opt_get_grads add them -- one launch less per iteration.) */
int fdcap_opt_backward_fit2d(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, int32_t log_terms, void* stream);
/* What the stage struct does not hold of SMPLify-X's objective (fdcap_fit2d_stage keeps its layout).  The BENDING PRIOR on the body
 * joints (SMPLify-X's angle prior: elbows and knees must not bend backwards; csrc/fdc_fit2d.h):
 *     w_bend * sum_t exp(sign[t] * aa_{joint[t]}[axis[t]])^2
 * with aa_j the axis-angle of body joint j in 1..21 as vposer.decode(z, 'aa') returns it; w_bend enters as it is (SMPLify-X: 3.17 x
 * the stage's body-pose prior weight), the terms are the caller's (elbows about y, knees about x in SMPL-X: fdcap_amd.innerfit).  It
 * joins the priors (losses_d [1], the per-frame objective of fdcap_opt_fit2d_lbfgs) on the 23-joint and the mapped data term alike,
 * by one small launch per evaluation; with n_bend = 0 or w_bend = 0 there is no such launch and every result has the bits it had.
 * w_jaw: the weights of the prior on a free jaw (fdcap_opt_set_jaw), sum_c (w_jaw[c] * jaw[c])^2, which joins the priors as well;
 * without a free jaw the term is exactly zero and nothing reads them. */
#define FDCAP_MAX_BEND_TERMS 8
typedef struct fdcap_fit2d_extra {
    float w_jaw[3];
    float w_bend;
    int32_t n_bend;                               /* 0 .. FDCAP_MAX_BEND_TERMS */
    int32_t joint[FDCAP_MAX_BEND_TERMS];          /* 1 .. 21 */
    int32_t axis[FDCAP_MAX_BEND_TERMS];           /* 0 .. 2 */
    float sign[FDCAP_MAX_BEND_TERMS];             /* +1 / -1: the direction that is penalised */
} fdcap_fit2d_extra;
/* Holds until the next call; extra = NULL: off.  FDCAP_E_ARG: more than FDCAP_MAX_BEND_TERMS terms, a joint outside 1..21, an axis
 * outside 0..2, a non-finite weight or sign.  FDCAP_E_STATE: no optimiser, a batch of clips or one rank's share of a clip (as the
 * rest of the inner fit). */
int fdcap_opt_set_fit2d_extra(fdcap_ctx* ctx, const fdcap_fit2d_extra* extra);
/* A FREE JAW for the mapped data term (csrc/fdc_keypoints.h): one axis-angle per frame, jaw_d DEVICE [n_local, 3], copied; NULL: fixed
 * at zero again, the model every other call of this library uses.  SMPL-X's joint 22 is a leaf of the tree, so the jaw changes the
 * pose-feature block of that joint and its skinning transform and nothing else: the vertices skinned to the jaw follow it, no joint
 * moves.  From here on fdcap_debug_keypoints3d, fdcap_opt_backward_fit2d and fdcap_opt_fit2d_lbfgs (81 unknowns per frame: the row,
 * then the jaw) honour it, fdcap_opt_step_x steps it with the rows' lr and step number, fdcap_opt_reset_adam zeroes its moments too.
 * fdcap_opt_get_results and the clip-level modes keep the jaw at zero (the self-interpenetration term too, unless
 * fdcap_opt_set_fit2d_collision_face opts in); the full-mesh operators
 * take it, and the expression coefficients, through their `_face` forms (fdcap_smplx_forward_face, fdcap_body_forward_face,
 * fdcap_world_mesh_face: what turns fdcap_opt_get_jaw / fdcap_opt_get_expression back into vertices).
 * FDCAP_E_ARG: a model whose joint 22 has a child.  FDCAP_E_STATE: no optimiser, a batch of clips or one rank's share of a clip; and
 * from an evaluation with a free jaw on the 23-joint layout (fdcap_opt_set_keypoints: no keypoint there follows the jaw). */
int fdcap_opt_set_jaw(fdcap_ctx* ctx, const float* jaw_d, void* stream);
/* the jaw and -- optional -- the objective's gradient with respect to it at the last evaluation, DEVICE [n_local, 3] each (either may
 * be NULL, not both).  FDCAP_E_STATE: no free jaw; djaw_d before an evaluation. */
int fdcap_opt_get_jaw(fdcap_ctx* ctx, float* jaw_d, float* djaw_d, void* stream);
/* FREE EXPRESSION COEFFICIENTS for the mapped data term (csrc/fdc_keypoints.h): ten per frame, expr_d DEVICE [n_local, 10], copied; NULL:
 * fixed at zero again, the model every other call of this library uses.  SMPL-X treats them as ten more shape directions (shapedirs'
 * columns 10..19 of fdcap_model_desc): v_shaped = v_template + S betas + E psi with the joints regressed from v_shaped -- the exact
 * model, evaluated as a correction of the pose kernels' chain inside the data term's kernel.  From here on fdcap_debug_keypoints3d,
 * fdcap_opt_backward_fit2d, fdcap_opt_fit2d_frame_loss and fdcap_opt_fit2d_lbfgs (88 unknowns per frame, 91 with a free jaw: the row,
 * psi, then the jaw; fdcap_opt_fit2d_lbfgs_rolled_back counts as before and psi is rolled back with its row) honour them,
 * fdcap_opt_step_x steps them with the rows' lr and step number, fdcap_opt_reset_adam zeroes their moments too.  The camera stage
 * (fdcap_opt_backward_fit2d_camera, fdcap_opt_fit2d_camera_lbfgs) ignores them and leaves them where they are; fdcap_opt_get_results,
 * the clip-level modes and -- without fdcap_opt_set_fit2d_collision_face -- the self-interpenetration term keep psi = 0 (the full-mesh
 * operators take it through their `_face` forms).  fdcap_fit2d_select does not carry them: gather them with chosen_d.
 * FDCAP_E_ARG: a model with a joint in front of its parent.  FDCAP_E_STATE: no optimiser, a batch of clips, one rank's share of a clip,
 * a model with num_shape < 20; from an evaluation on the 23-joint layout (fdcap_opt_set_keypoints: the correction runs in the mapped
 * term's kernel); and together with the self-interpenetration term, at the evaluation or in fdcap_opt_set_fit2d_collision (the
 * full-mesh pass skins with the transforms the pose kernels wrote, at psi = 0). */
int fdcap_opt_set_expression(fdcap_ctx* ctx, const float* expr_d, void* stream);
/* the coefficients and -- optional -- the objective's gradient with respect to them at the last evaluation, DEVICE [n_local, 10] each
 * (either may be NULL, not both: FDCAP_E_ARG).  FDCAP_E_STATE: no free expression; dexpr_d before an evaluation. */
int fdcap_opt_get_expression(fdcap_ctx* ctx, float* expr_d, float* dexpr_d, void* stream);
/* the weight of the prior w_expr^2 |psi|^2, which joins losses_d [1] and every frame's objective; holds until the next call (0 at
 * fdcap_opt_create); without free expression coefficients nothing reads it.  FDCAP_E_ARG: a non-finite weight.  FDCAP_E_STATE: as
 * fdcap_opt_set_expression's first three. */
int fdcap_opt_set_expression_prior(fdcap_ctx* ctx, float w_expr);
/* The inner fit's self-interpenetration term on the mesh of fdcap_set_collision_mesh; holds until the next call; params = NULL or
 * w_coll == 0: off, and then not one launch or argument of an evaluation differs.  With it every evaluation (fdcap_opt_backward_fit2d,
 * fdcap_opt_fit2d_lbfgs, fdcap_opt_fit2d_frame_loss) runs, after the pose forward and the data term, the full-mesh blend and skinning
 * forward over the n_local rows, fdcap_collision_eval's steps on those world vertices (every_pair honoured) and the skinning and
 * blend backward; the sums join the data term's before the bending prior and the pose backward.  A frame's value joins its
 * objective (what the L-BFGS driver sees); log_terms != 0: losses_d [FDCAP_LOSS_FIT2D_COLLISION] = the frames' values, a slot the
 * inner fit otherwise leaves at zero.  FDCAP_E_ARG: what fdcap_collision_eval refuses in params.  FDCAP_E_STATE: no optimiser, a
 * batch of clips, one rank's share of a clip, no registered mesh, a FREE JAW (here, or at the evaluation when the jaw was freed
 * later: the full-mesh pass skins with the transforms the pose kernels wrote, in which the jaw is shut). */
#define FDCAP_LOSS_FIT2D_COLLISION 4
int fdcap_opt_set_fit2d_collision(fdcap_ctx* ctx, const fdcap_collision_params* params);
/* OPT-IN: the term may follow a free jaw and free expression coefficients.  on != 0: fdcap_opt_set_fit2d_collision accepts both, and
 * the term's full-mesh pass skins the FITTED face (csrc/fdc_face_mesh.h: the corrected transforms, the jaw's pose-feature block, E psi on the
 * offsets); its share of d psi and of the jaw's two gradient parts joins the data term's in a fixed order, in the arrays fdcap_opt_get_jaw /
 * fdcap_opt_get_expression, fdcap_opt_step_x and fdcap_opt_fit2d_lbfgs read, and fdcap_opt_fit2d_frame_loss includes the term.  0 (the
 * default): a free jaw and free psi are refused as above, and with the term off or the face fixed not one launch or argument of an
 * evaluation differs.  Still FDCAP_E_STATE: no optimiser, a batch of clips, one rank's share of a clip; and, from an evaluation, a free
 * jaw or psi on the 23-joint layout. */
int fdcap_opt_set_fit2d_collision_face(fdcap_ctx* ctx, int32_t on);
int fdcap_opt_reset_adam(fdcap_ctx* ctx, void* stream);

/* ---- batched L-BFGS with a strong-Wolfe line search (csrc/fdc_lbfgs.h) ----
 * SMPLify-X fits every frame with L-BFGS (its `optimizer.step(closure)` loop with line_search_fn = "strong_wolfe"), not Adam;
 * neither is in the reference repository (README.md:14-17 delegates the per-frame fit).  The algorithm is the published one
 * of torch.optim.LBFGS, restated as a resumable state machine per problem: n_problems INDEPENDENT problems of `dim` <= 128
 * unknowns advance together, one launch between two evaluations of the caller's objective.
 *   max_iter / max_eval / history / lr / tolerance_grad / tolerance_change: torch.optim.LBFGS's arguments (max_eval <= 0:
 *       max_iter * 5 / 4; history <= 128);
 *   max_ls: extrapolation / zoom rounds of ONE line search after its first evaluation, i.e. at most max_ls + 1 evaluations per
 *       search, whatever the step has already spent (the fixed 25 of older torch.  Current torch caps a search at the step's
 *       remaining evaluations instead, max_eval - evaluations so far: the same decisions unless a search reaches the smaller cap);
 *   max_steps, ftol, gtol: SMPLify-X's loop around optimizer.step(): at most max_steps calls, stop when the loss at the start
 *       of two successive calls differs by <= ftol relative to max(|a|, |b|, 1) or every gradient entry is below gtol
 *       (max_steps = 1, ftol = gtol = 0: exactly one optimizer.step()). */
typedef struct fdcap_lbfgs_config {
    int32_t dim, history, max_iter, max_eval, max_steps, max_ls;
    float lr, tolerance_grad, tolerance_change, ftol, gtol;
} fdcap_lbfgs_config;
typedef struct fdcap_lbfgs fdcap_lbfgs;
int fdcap_lbfgs_create(int32_t n_problems, const fdcap_lbfgs_config* cfg, fdcap_lbfgs** out);
void fdcap_lbfgs_destroy(fdcap_lbfgs* opt);
/* forget everything (a fresh optimiser, as SMPLify-X builds for every stage) */
int fdcap_lbfgs_reset(fdcap_lbfgs* opt, void* stream);
/* One round.  In: f_d DEVICE [n_problems], g_d DEVICE [n_problems rows of g_stride floats] = objective and gradient at the
 * points in x_d DEVICE [n_problems rows of x_stride floats] (the first call after create / reset: at the starting points).
 * Out: x_d = the next points to evaluate (for a finished problem: its result, no longer touched); n_active_d DEVICE int32 (may
 * be NULL) = problems that want another round.  Call until n_active is 0. */
int fdcap_lbfgs_advance(fdcap_lbfgs* opt, float* x_d, int32_t x_stride, const float* f_d, const float* g_d, int32_t g_stride,
                        int32_t* n_active_d, void* stream);
/* A caller that stops before n_active is 0 (a round budget): every unfinished problem's x row holds a line-search TRIAL point
 * (bracketing extrapolates up to 10x per step), not an accepted one.  This puts the last accepted point back (the one `loss` of
 * fdcap_lbfgs_get_stats belongs to), marks those problems finished and counts them in n_unfinished_d (DEVICE int32, may be NULL). */
int fdcap_lbfgs_finalize(fdcap_lbfgs* opt, float* x_d, int32_t x_stride, int32_t* n_unfinished_d, void* stream);
/* per problem, DEVICE, any may be NULL: iterations [n] (L-BFGS directions taken), evaluations [n] (objective calls consumed),
 * loss [n] (objective at the accepted point) */
int fdcap_lbfgs_get_stats(fdcap_lbfgs* opt, int32_t* iterations_d, int32_t* evaluations_d, float* loss_d, void* stream);

/* The inner fit of one stage with L-BFGS instead of Adam: rounds of (forward, fit2d loss, backward, fdcap_lbfgs_advance on the
 * n_local rows of body_rotation_rec) until every frame has stopped or max_rounds evaluations were made; a fresh optimiser per
 * call; cfg->dim is ignored (78).  *rounds_out (may be NULL) = evaluations made.  Synchronises `stream` every few rounds (to
 * read the number of frames still running) and before it returns.  Frames still inside a line search when max_rounds is reached
 * are rolled back to their last accepted point (fdcap_lbfgs_finalize): the rows returned are never trial points.
 * Outer stop, as built: relative change of the loss between two step() calls <= ftol, or max|g| < gtol with g the gradient at the
 * ACCEPTED point.  (SMPLify-X tests param.grad as the last line-search evaluation left it; with strong Wolfe that is the accepted
 * point's gradient except when the search ends on its evaluation cap.  oracle/innerfit.py makes the same choice.) */
int fdcap_opt_fit2d_lbfgs(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, const fdcap_lbfgs_config* cfg, int32_t max_rounds,
                          int32_t* rounds_out, void* stream);
/* fdcap_lbfgs_get_stats of the last fdcap_opt_fit2d_lbfgs call, per frame [n_local] (FDCAP_E_STATE before the first) */
int fdcap_opt_fit2d_lbfgs_stats(fdcap_ctx* ctx, int32_t* iterations_d, int32_t* evaluations_d, float* loss_d, void* stream);
/* *n_frames (HOST) = the frames the last fdcap_opt_fit2d_lbfgs call found inside a line search when max_rounds ran out and rolled back
 * to their last accepted point (rows, and the jaw when it is free); 0 when every frame had finished.  FDCAP_E_STATE before the first call. */
int fdcap_opt_fit2d_lbfgs_rolled_back(fdcap_ctx* ctx, int32_t* n_frames);

/* ---- the inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h): SMPLify-X's depth guess, camera stage and 180-degree twin ----
 * Outside the reference repository like the rest of the inner fit; every constant is the caller's (defaults: innerfit.py DEFAULT_INIT).
 * A SLOT is an index into a frame's keypoint array: with fdcap_opt_set_keypoints the joint itself (0..22), with a keypoint map an
 * entry of the map that is an SMPL-X joint.
 *   edge [n_edge <= 4][2] : the torso edges of the depth guess, z = mean |G_a.t - G_b.t| / mean |((u_a - u_b) / fx, (v_a - v_b) / fy)|
 *                           over the edges whose two confidences exceed conf_thr; no such edge (or a mean image length below 1e-6):
 *                           z = default_depth and valid = 0
 *   torso [n_torso <= 8]  : the keypoints of the camera stage's objective
 *                           w_data^2 sum_{k, conf_k > conf_thr} [(u_k - kp_k.u)^2 + (v_k - kp_k.v)^2] + w_depth^2 (cam_t.z - z0)^2
 *                           over global_orient (6 columns) and camera_translation (3) alone; z0: camera_translation's z at set-up
 *   shoulder [2]          : side_view = both detected and closer than side_view_px in the image
 * The three calls that take it return FDCAP_E_STATE for a batch of clips, a shard of a clip or before keypoints are set, FDCAP_E_ARG for
 * n_edge outside 1..4, n_torso outside 1..8, a slot outside the keypoint array or on a surface point, or a non-finite setting. */
typedef struct fdcap_fit2d_init {
    int32_t n_edge, edge[4][2], n_torso, torso[8], shoulder[2];
    float conf_thr, default_depth, side_view_px, w_data, w_depth;
} fdcap_fit2d_init;
/* One pose forward, then per frame camera_translation = (0, 0, z) -- nothing else of a row is written -- and, DEVICE [n_local], each
 * optional: z_d (float), valid_d and side_view_d (int32). */
int fdcap_opt_fit2d_guess(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, const fdcap_fit2d_init* init, float* z_d, int32_t* valid_d,
                          int32_t* side_view_d, void* stream);
/* One evaluation of the camera stage's objective and its gradient: nine columns of the rows' gradient, the other 69 written as exact
 * zeros; fdcap_opt_get_grads / fdcap_opt_step_x work after it as after fdcap_opt_backward_fit2d (Adam from zero moments leaves a
 * zero-gradient column where it is).  The body model runs at SET-UP only -- the first evaluation after fdcap_opt_set_inputs, after
 * any other call that runs the model (fdcap_opt_fit2d_guess, fdcap_opt_backward_fit2d, ...: whatever may step the other columns), after a
 * change of the torso list, or any call with log_terms & 2 -- which stores each torso joint's offset from the pelvis in the root's
 * frame and z0.  A caller who writes the registered rows directly changes only the nine columns in between, or asks for set-up.  log_terms & 1: losses_d [0] = the
 * data term, [1] = the depth term.  A free jaw is ignored and stays where it is. */
int fdcap_opt_backward_fit2d_camera(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, const fdcap_fit2d_init* init, int32_t log_terms, void* stream);
/* The camera stage with L-BFGS, shaped like fdcap_opt_fit2d_lbfgs (same polling, roll-back, fdcap_opt_fit2d_lbfgs_stats and
 * fdcap_opt_fit2d_lbfgs_rolled_back afterwards): rounds of one evaluation (the first with set-up where it is due, as above) +
 * fdcap_lbfgs_advance on the 78-wide rows.  A column
 * whose gradient is exactly zero in every round keeps a zero direction, so the 69 fixed columns keep their bits. */
int fdcap_opt_fit2d_camera_lbfgs(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, const fdcap_fit2d_init* init, const fdcap_lbfgs_config* cfg,
                                 int32_t max_rounds, int32_t* rounds_out, void* stream);
/* The FULL objective of fdcap_opt_backward_fit2d per frame at the current rows, under the current keypoints, map, jaw and
 * fdcap_opt_set_fit2d_extra settings: floss_d DEVICE [n_local].  One evaluation (the gradients are that evaluation's afterwards). */
int fdcap_opt_fit2d_frame_loss(fdcap_ctx* ctx, const fdcap_fit2d_stage* stage, float* floss_d, void* stream);
/* rows75_d DEVICE [n, 75], in place: global_orient = log(R(global_orient) R_y(pi)), the body turned 180 degrees about its y. */
int fdcap_fit2d_flip_orient(float* rows75_d, int32_t n, void* stream);
/* The better of a frame's two fits.  rows_d [n + m, 75] and loss_d [n + m]: problems 0..n-1 the frames, problem n + i a twin of frame
 * src_d [i] (int32 [m], ascending and unique; m may be 0, src_d then NULL); jaw_d [n + m, 3] optional with jaw_out_d [n, 3].  Per frame
 * the twin is taken iff its loss is strictly lower, a NaN loss counting as +inf (both NaN: the frame's own): rows_out_d [n, 75],
 * chosen_d int32 [n] (0 / 1, optional).  All DEVICE. */
int fdcap_fit2d_select(const float* rows_d, const float* loss_d, const int32_t* src_d, int32_t n, int32_t m, const float* jaw_d,
                       float* rows_out_d, float* jaw_out_d, int32_t* chosen_d, void* stream);

/* Multi-GPU iteration tail with ONE collective per iteration (instead of an all-reduce before the
 * step and point-to-point halo messages after it):
 *   fdcap_opt_step_rows_and_pack : Adam on body_rotation_rec / camera_ext of the owned rows, then writes
 *       send_d [fdcap_exchange_len()] = this rank's first two + last two owned rows (x | camera_ext)
 *       and its d loss / d scale partial;
 *   (caller: all-gather send_d over the ranks into gathered_d [world, fdcap_exchange_len()]);
 *   fdcap_opt_unpack_and_step_scale : fills the halo rows from ranks rank-1 / rank+1, sums the scale
 *       gradient over ranks in rank order (bit-identical on every rank) and applies Adam to scale. */
int fdcap_opt_step_rows_and_pack(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, float* send_d, void* stream);
int fdcap_opt_unpack_and_step_scale(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, const float* gathered_d,
                                    int32_t rank, int32_t world, void* stream);
int32_t fdcap_exchange_len(void);

/* ---- the exchange INSIDE the library (SURVEY 8b "halo_exchange", 8e) -----------------------------------------------------
 * The reference has no distributed code; this is the communicator of the frame-sharded optimiser for callers that are not
 * Python (and for Python: two calls per iteration instead of five, no stream hand-over).  RCCL is bound at run time
 * (dlopen librccl.so.1; FDCAP_RCCL_LIB names another file, tried first; with FDCAP_RCCL_LIB_ONLY=1 nothing else is tried):
 * FDCAP_E_COMM when it is not there, the loader's message in fdcap_comm_last_error (a NULL context, or a context without a
 * message of its own, returns the process-wide loader message).  One communicator per context, created
 * on the calling thread's current HIP device; every rank of the job calls fdcap_comm_create with the SAME id.
 *   fdcap_comm_unique_id : `id128` [FDCAP_UNIQUE_ID_BYTES] host bytes; rank 0's go to the other ranks out of band (any rank may
 *                          call it: it is also the cheap test that librccl can be bound in this process)
 *   fdcap_comm_create    : ncclCommInitRank (collective: blocks until all `world` ranks arrive)
 *   fdcap_opt_halo_exchange : halo rows <- the neighbours' boundary rows as they are (before the first iteration, after
 *                          fdcap_opt_import_state, after each fdcap_opt_step_x of mode 'local')
 *   fdcap_opt_exchange   : the sharded iteration tail, whole -- fdcap_opt_step_rows_and_pack, ONE ncclAllGather of
 *                          fdcap_exchange_len() floats per rank on `stream`, fdcap_opt_unpack_and_step_scale -- in place of
 *                          fdcap_opt_step; same kernels, same bits as the caller-side sequence above
 *   fdcap_comm_allreduce_f64 : in-place sum over the ranks (the logged loss partial sums) */
int fdcap_comm_unique_id(uint8_t* id128);
int fdcap_comm_create(fdcap_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world);
int fdcap_comm_destroy(fdcap_ctx* ctx);
const char* fdcap_comm_last_error(fdcap_ctx* ctx);
int fdcap_opt_halo_exchange(fdcap_ctx* ctx, void* stream);
int fdcap_opt_exchange(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, void* stream);
/* The exchange measured on the communicator at hand: mean microseconds of `iters` whole tails (fdcap_opt_exchange) and of `iters` bare
 * ncclAllGather calls of the iteration's message, each train between two HIP events on `stream`.  Every rank must make the same
 * call; the optimiser's state is stepped `iters` times with the gradients it holds (call it after the fit).  Synchronises. */
int fdcap_opt_time_exchange(fdcap_ctx* ctx, int32_t iters, float* us_exchange, float* us_allgather, void* stream);
int fdcap_comm_allreduce_f64(fdcap_ctx* ctx, double* buf_d, int32_t n, void* stream);
/* Overlap of the exchange with the next forward.  Issued between the two calls above, i.e. while the all-gather is in
 * flight: the part of iteration ii's forward (ii = the NEXT iteration; log_terms as its fdcap_opt_backward will get) that needs
 * neither `scale` nor the halo rows -- decoder, pose state and the contact set's pose-blend product of the owned rows
 * (global_optimization.py:270-283 up to `verts * scale`, :284).  The next fdcap_opt_backward(ii) then only decodes the halo
 * rows and refreshes the scale-dependent outputs (two nearly empty launches) before it goes on; parameters are bit-identical
 * to the schedule without this call.  Anything that changes the owned rows in between (a step, fdcap_opt_import_state) drops
 * what ran ahead. */
int fdcap_opt_forward_ahead(fdcap_ctx* ctx, int32_t ii, int32_t first_phase2_iter, int32_t log_terms, void* stream);

/* Results: body_rec75_d [n_local,75] (= convert_to_3D_rot, :633), scale_d [1], cam_ext_d [n_local,16].
 * A batch of K clips: [K*N,75], [K] (clip k's scale at k), [K*N,16]. */
int fdcap_opt_get_results(fdcap_ctx* ctx, float* body_rec75_d, float* scale_d, float* cam_ext_d,
                          void* stream);
void fdcap_opt_destroy(fdcap_ctx* ctx);

/* World-space contact vertices / joints of the current state (testing + viewers):
 * verts_d [n_local,nc,3] (optional), joints_d [n_local,23,3] (optional). */
int fdcap_opt_forward_world(fdcap_ctx* ctx, float* verts_d, float* joints_d, void* stream);
/* Nearest-neighbour result of the last contact forward (testing): dist_d [n_local,nc] squared
 * distances, idx_d [n_local,nc] scene indices.  The optimiser seeds each search with the previous
 * call's idx (an exact upper bound that only prunes; FDCAP_NN_SEED=0 disables).
 * A batch of clips of several scenes (fdcap_opt_create_clips_scenes): both arrays stay flat per query, and idx is an index into
 * the scene of the query's OWN clip, in that scene's input order (below that slot's point count, not slot 0's). */
int fdcap_opt_get_contact(fdcap_ctx* ctx, float* dist_d, int32_t* idx_d, void* stream);
/* Gradients of the last fdcap_opt_backward (testing): dx_d [n_local,78], dcam_d [n_local,16]. */
int fdcap_opt_get_grads(fdcap_ctx* ctx, float* dx_d, float* dcam_d, void* stream);

/* Kernel-level timing of the full-mesh pose-blendshape GEMM ([rows,486] x posedirs
 * [486, 3V] on the fp32 matrix cores), HIP events on `stream`, mean milliseconds per launch. */
int fdcap_time_blend_gemm(fdcap_ctx* ctx, int32_t rows, int32_t iters, float* ms, void* stream);

/* The loop's dense contraction on its own (testing): C_d[M,N] (row-major, ldc) = A_d[M,K] (row-major, lda) x B,
 * B a HOST array, element (k, n) at B_h[k * sk + n * sn] -- re-laid out in MFMA fragment order exactly as the
 * context does for the VPoser weights and the blend directions, then run by the kernel the loop uses
 * (v_mfma_f32_16x16x4_f32: every output is the k-ordered fp32 fmaf chain).  Synchronises `stream`. */
int fdcap_panel_gemm(const float* A_d, int32_t lda, int32_t M, int32_t K, const float* B_h, int64_t sk, int64_t sn, int32_t N,
                     float* C_d, int32_t ldc, void* stream);

/* In-loop timing of the Chamfer NN launch: while enabled (max_launches > 0), every contact forward of the optimiser is
 * bracketed by two HIP events on its launch stream (up to max_launches of them; 0 disables and resets).
 * fdcap_opt_nn_timing_read waits for the recorded events and returns the mean milliseconds per launch and their number:
 * the launch as the loop really issues it, iteration by iteration (`roofline.ms_per_launch` of bench.py). */
int fdcap_opt_nn_timing(fdcap_ctx* ctx, int32_t max_launches);
int fdcap_opt_nn_timing_read(fdcap_ctx* ctx, float* mean_ms, int32_t* launches);

/* Tests / diagnosis: which queries share a wave of the in-loop Chamfer NN launch (scheduling only: every mode gives the same
 * bits).  mode 0 (default): grouped by the k-d quarter of each query's current neighbour, rebuilt after the seeding launch and
 * every 32 launches; 1: query order (32 consecutive query indices per wave); 2: perm_h [n] (n = frames x contacts, a
 * permutation: wave slot s serves query perm_h[s]), kept until the next call.  Drops the kept work lists.  Synchronises the device. */
int fdcap_debug_nn_query_order(fdcap_ctx* ctx, int32_t mode, const int32_t* perm_h, int32_t n);
/* Tests / diagnosis: the in-loop search's neighbour records of the last contact forward, [n_local, nc, 4] floats in the caller's
 * contact order: {x, y, z} of the neighbour fdcap_opt_get_contact reports and the bits of its position in the sorted scene.
 * FDCAP_E_STATE when the last contact forward's search took a form that keeps no records (the plain or the staged scan). */
int fdcap_debug_nn_records(fdcap_ctx* ctx, float* rec4_d, void* stream);
/* Tests / diagnosis: which paths this optimiser's launches took since fdcap_opt_create[_clips].  out4[0]: search launches that
 * wrote only the changed neighbour records; out4[1]: skinning backwards that formed the world vertices and distances themselves;
 * out4[2]: search launches under a query order; out4[3]: rebuilds of the query order. */
int fdcap_debug_contact_diet(fdcap_ctx* ctx, int32_t* out4);
/* Tests / diagnosis: one-wave search launches since fdcap_opt_create[_clips] by the lanes per listed box they were launched with
 * (FDCAP_NN_BOX_LANES): out4[0] by each stage's count, out4[1] / [2] / [3] forced 2 / 4 / 8. */
int fdcap_debug_nn_box_tests(fdcap_ctx* ctx, int32_t* out4);
/* Tests / diagnosis: what the skinning backward of the last fdcap_opt_backward that had a contact gradient left, per frame, into DEVICE
 * arrays: dA_d [n_local][55 * 12] (the rows of joints below *ja_hi_out -- a HOST int -- are written), dtransl_d [n_local][3], dMv_d
 * [n_local][12], dsv_d [n_local], dVoff_d [n_local][contacts][3] (contacts in slot order).  reference != 0: instead, the same state --
 * parameters, pose offsets, transforms, neighbours -- run once more through the contact-set kernel with every wave sum formed on its
 * own (lane 0 stores), as every build before the packed sums did, into buffers of its own: the two must agree byte for byte.
 * reference needs a contact set of at most 512 vertices (else FDCAP_E_STATE).  FDCAP_E_STATE also when the last backward of this
 * optimiser had no contact gradient, or none has run since it was created.  Synchronises `stream`. */
int fdcap_debug_skin_bwd_sums(fdcap_ctx* ctx, int32_t reference, float* dA_d, float* dtransl_d, float* dMv_d, float* dsv_d, float* dVoff_d,
                              int32_t* ja_hi_out, void* stream);
/* Tests / diagnosis: perm_h [n = contacts]: internal contact slot -> position in the caller's id array (fdcap_set_contact_ids);
 * a frame's queries lie in idx / seedpt in slot order.  Synchronous copy. */
int fdcap_debug_contact_perm(fdcap_ctx* ctx, int32_t* perm_h, int32_t n);

/* Tests / diagnosis: the sort behind mode 0 above on its own, on the launch path the optimiser uses.  pos_h [nq]: the position
 * of each query's neighbour in the sorted scene (-1: none); the key is min(pos >> 7, 0xFFFF), 0xFFFF without a neighbour.
 * perm_out [nq] receives the order (stable: by key, ties by query index).  hdr_io [hdr_len >= groups] stands for the kept-list
 * headers: uploaded as given, returned as the rebuild leaves them (the first `groups` entries -1, the rest untouched).
 * Needs no optimiser; allocates and frees its own device buffers.  Synchronises `stream`. */
int fdcap_debug_nn_query_sort(fdcap_ctx* ctx, const int32_t* pos_h, int32_t nq, int32_t groups, int32_t hdr_len, int32_t* hdr_io,
                              int32_t* perm_out, void* stream);
/* ... under the key min(pos >> shift, 0xFFFF), shift 5, 6 or 7 (r21: the order's key is the neighbour's 32-point tile wherever the
 * scene's tiles fit 16 bits; else FDCAP_E_ARG).  fdcap_debug_nn_query_sort is this call with shift 7. */
int fdcap_debug_nn_query_sort_shift(fdcap_ctx* ctx, const int32_t* pos_h, int32_t nq, int32_t groups, int32_t hdr_len, int32_t* hdr_io,
                                    int32_t* perm_out, int32_t shift, void* stream);
/* Tests / diagnosis (r21): the streaming search's scheduling choices within one build (scheduling only: the same bits), process-wide
 * like fdcap_set_nn_kernel.  key_shift: the query order's key is the neighbour's position in the sorted scene >> key_shift -- 5, 6 or
 * 7; 0: automatic, the finest of them whose keys stay below 0xFFFF for the scene's size.  items_per_chunk: work items per 512-point
 * chunk of the one-wave form -- 4 (quarters), 8 (64-point eighths; quarters all the same where 8 x chunks exceeds the 16-bit ids) or 0
 * (automatic: 8 where the ids fit and the launch has more than 2^21 queries); anything else FDCAP_E_ARG.  Drops the kept work lists of this context (the optimiser's, every
 * segment of a batch of scenes, and fdcap_chamfer_fwd_scene's, which starts over); an optimiser's order is rebuilt after its next
 * search launch.  Other contexts of the process must not hold kept lists across the call.  Synchronises the device. */
int fdcap_debug_nn_search_form(fdcap_ctx* ctx, int32_t key_shift, int32_t items_per_chunk);

/* In-loop timing of EVERY launch of an iteration (r6; bench.py's roofline.per_kernel[].us_live): while enabled (max_events > 0) the
 * optimiser records a HIP event on its launch stream at every boundary between two launches of an iteration (up to max_events
 * events in all; 0 disables and resets) -- one fit of 500 iterations records ~4100.  fdcap_opt_launch_timing_read waits for them and
 * returns, per stage and per phase of the fit, the mean microseconds from the event before the stage's launch(es) to the event
 * after them (so ~1 us of dependent-launch gap is inside every figure) and the number of samples:
 *   mean_us[FDCAP_LT_NUM * phase + stage], counts[...]   phase 0: iterations whose loss has the contact term (ii < P), 1: the others.
 * The events themselves cost a few microseconds per iteration: a fit timed this way is for the per-kernel table, never `value`. */
#define FDCAP_LT_VPOSER_FWD 0    /* VPoser decode (+ the deferred Adam step of the rows) */
#define FDCAP_LT_POSE_FWD 1      /* rotations, joint regression, kinematic chain, world joints */
#define FDCAP_LT_CONTACT_FWD 2   /* contact set: blend product + skinning + world transform (one launch at clip size, else two) */
#define FDCAP_LT_CHAMFER_NN 3    /* Chamfer nearest-neighbour search (+ its seeding launch in a fit's first iteration) */
#define FDCAP_LT_SKIN_BWD 4      /* contact robustifier + skinning backward */
#define FDCAP_LT_BLEND_BWD 5     /* data gradient of the blend product */
#define FDCAP_LT_POSE_BWD 6      /* chain / rotation backward + parameter-space losses (+ the reprojection term, fdcap_opt_set_reproj) */
#define FDCAP_LT_VPOSER_BWD 7    /* VPoser data gradient (+ the `scale` step) */
#define FDCAP_LT_NUM 8
int fdcap_opt_launch_timing(fdcap_ctx* ctx, int32_t max_events);
int fdcap_opt_launch_timing_read(fdcap_ctx* ctx, float* mean_us /* [2 * FDCAP_LT_NUM] */, int32_t* counts /* [2 * FDCAP_LT_NUM] */);

/* Kernel-level timing of the Chamfer NN launch for the roofline line: runs `iters` launches of
 * the optimiser's Chamfer forward on `stream` between two HIP events and returns the mean
 * milliseconds per launch in *ms.  brute_force = 1: every (query, scene point) pair is visited
 * (no seed, no chunk bounds) -- the launch the algorithmic byte count describes; 0: the launch
 * exactly as the loop issues it in steady state (seeded, chunk-culled). */
int fdcap_opt_time_chamfer(fdcap_ctx* ctx, int32_t iters, int32_t brute_force, float* ms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDCAP_H */
