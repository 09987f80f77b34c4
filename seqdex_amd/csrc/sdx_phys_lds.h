// sdx_phys_lds.h - private to sdx_physics.hip (included by it only, in its fixed order): constants, wave hand-offs, the LDS layout and its overlays, clock / ablation macros
#pragma once

#define NL SDX_NLINK
#define ND SDX_NDOF
#define NF SDX_NFREE
#define HP 24                 // padded row stride of the 23x23 matrices in LDS
#define MAXC SDX_MAXC
#define MAXP SDX_MAXP
#define GL 4                  // lane spacing of the bricks' bK owners (solve: pass_setup()); the gather's lanes per brick are chosen per solve (gtab)
#define NBODY (NF + NL + 1)   // bricks, links, the static world
#define BODY_W (NF + NL)      // body id of the static world inside the kernel (SDX_BODY_STATIC = 255 outside)
// link frame origins / twists are rows NF.. of the body table: S.bp[NF + k], S.bv[NF + k], S.bw[NF + k]

// LDS written by one lane and read by another lane of the SAME wave without a workgroup barrier: the wave runs in lockstep and the
// LDS executes one wave's operations in order, so only the compiler must be kept from moving accesses across this point
#define WAVE_SYNC()                                         \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
  } while (0)

// Barrier among the waves that hold threads 0 .. nthreads-1 only (whole waves; every one of them calls it): a wave announces itself on an
// LDS counter once its LDS writes have completed and waits until `target` arrivals have been counted.  The counter is monotonic - the
// caller passes (waves) x (number of calls so far) - and the LDS executes the operations of a CU in issue order, so a wave that has seen
// the count reads what the others wrote before they signalled.  Used where a few waves have a dependent stage of their own while the rest
// of the block is busy with independent work (solver loop: link gather -> robot section beside the brick gather); the waves of a
// workgroup are resident together, so the wait cannot deadlock.
#ifdef HIPEMU
#define WAVES_BARRIER(ctr, target, nthreads) hipemu::group_barrier(nthreads)
#else
__device__ __forceinline__ void waves_barrier(int* ctr, int target) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
}
#define WAVES_BARRIER(ctr, target, nthreads) waves_barrier((ctr), (target))
#endif
// One wave tells the others that its LDS results up to here are complete (flag = a value that only grows); the others wait for it.
#ifdef HIPEMU
// (the emulator runs wave 0 up to its next workgroup barrier before any other wave: the flag is always set when a waiter looks)
#define WAVE_SIGNAL(flag, value) (*(flag) = (value))
#define WAVES_WAIT(flag, value) do { if (*(flag) < (value)) __builtin_trap(); } while (0)
#else
__device__ __forceinline__ void wave_signal(int* flag, int value) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void waves_wait(int* flag, int value) {
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < value) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
}
#define WAVE_SIGNAL(flag, value) wave_signal((flag), (value))
#define WAVES_WAIT(flag, value) waves_wait((flag), (value))
#endif

__constant__ float c_samp[SDX_NSAMP][3] = {
    {1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}, {-1, 1, 1}, {1, -1, 1}, {1, 1, -1},
    {0, -1, -1}, {0, 1, -1}, {0, -1, 1}, {0, 1, 1}, {-1, 0, -1}, {1, 0, -1}, {-1, 0, 1}, {1, 0, 1},
    {-1, -1, 0}, {1, -1, 0}, {-1, 1, 0}, {1, 1, 0},
    {-0.5f, -1, -1}, {0.5f, -1, -1}, {-0.5f, 1, -1}, {0.5f, 1, -1}, {-0.5f, -1, 1}, {0.5f, -1, 1}, {-0.5f, 1, 1}, {0.5f, 1, 1}};

struct PhysLds {
  // robot
  float q[ND], qd[ND + 1], qdb[ND + 1], tgt[ND], tau[ND];   // qd[ND] = 0: the padding dof of exhausted paths; qdb: the solver's second copy (read one, write the other)
  float lq[NL][4], la[NL + 1][3], lc[NL][3], lI[NL][6], lmass[NL];   // lmass: link masses (a per-lane global load inside the mass-matrix loop cost it 8 k cycles)
  float lal[NL + 1][3], lao[NL][3], lF[NL][3], lN[NL][3];   // velocity-product terms: angular / origin accelerations at zero qdd, inertial wrenches
  alignas(16) float A[ND][HP];      // H -> L -> Hinv
  uint32_t anc[NL];     // bit j: dof j lies on the path base -> link
  int par[NL + 1];      // parent link; [NL] = NL: the padding link of exhausted paths (zero rows of the body table)
  float cf[NL][3];
  // bricks (centre-of-box frame) and their per-brick constants
  // position / linear / angular velocity of EVERY body in one table: bricks 0..71 (centre of the box), links 72..95 (frame origin),
  // entry 96 = the static world (zeros): the solver's point velocities need no case distinction
  // bv / bw are 16-byte rows (one ds_read_b128 each).  INSIDE the solver loop row i of bv holds u_i = v_i - w_i x x_i, the velocity of the
  // body's material point at the world origin, so that a point velocity is u + w x p without the reference point (solve() converts on entry and exit)
  float bp[NBODY][3];
  alignas(16) float bv[NBODY][4];
  alignas(16) float bw[NBODY][4];
  float bq[NF][4];
  float bim[NF];               // inverse mass (target brick already scaled by 1 / seg_mass_scale)
  float bK[NF][6];             // world inverse inertia R diag(1/I) R^T of the substep (xx yy zz xy xz yz)
  // collision compounds by brick TYPE, in the brick's centre-of-mass frame: tsc / tsh the boxes (slabs of the convex
  // hull), tbc / tbh the bounding box, trad a radius about the centre of mass that contains it; hsc / hsh / hn: the hollow compound of
  // THIS env's target brick (walls, roof, upper part) when the scene asks for it (seg_hollow), else hn = 0
  unsigned char btype[NF];
  int tn[SDX_NBRICK_TYPES], hn;
  float tsc[SDX_NBRICK_TYPES][SDX_MAX_SUB][3], tsh[SDX_NBRICK_TYPES][SDX_MAX_SUB][3];
  float tbc[SDX_NBRICK_TYPES][3], tbh[SDX_NBRICK_TYPES][3], trad[SDX_NBRICK_TYPES], tii[SDX_NBRICK_TYPES][3];
  float hsc[SDX_MAX_SUB_HOLLOW][3], hsh[SDX_MAX_SUB_HOLLOW][3];
  float samp[SDX_NSAMP][3];    // copy of c_samp for per-lane sample indices (the manifold selection of pair_contacts)
  float qid[4];                // (0, 0, 0, 1): the orientation row a static body's box reads in load_box2
  // robot collision boxes in the world
  float rc[SDX_MAX_RBOX][3], rq[SDX_MAX_RBOX][4], rh[SDX_MAX_RBOX][3], rrad[SDX_MAX_RBOX];
  int rbl[SDX_MAX_RBOX];
  float sth[SDX_MAX_STATIC][3], stc[SDX_MAX_STATIC][3];   // bounding boxes of the static bodies as THIS env sees them
  int ssf[SDX_MAX_STATIC], ssn[SDX_MAX_STATIC];           // their boxes: rows [ssf, ssf + ssn) of sdx_scene_desc.static_sub_* (read from HBM: only the studded base plate has more than one)
  int acount[2][NF + 2];   // ACTIVE contacts per brick, [NF] on the whole robot, [NF + 1] = 0 (static world): one set is read while the other is counted; integer atomics
  int ecount[NF + NL];  // CSR build: contact sides per body
  float Qc[NL][12];     // per iteration: generalised impulse the contacts of link k apply to the s-th dof of its path (<= 11 dofs)
  uint32_t desc[ND];    // bit k: link k lies below dof j
  int nc, np, overflow, seg_brick, rebuilt, nrob;
  int rsync;            // arrivals at the robot waves' own barrier (solver loop), monotonic within a solve
  uint32_t gtab[NF];    // brick gather lanes of this solve: first lane | lanes << 9 (solve(): the balanced gather's row packing)
  int fkflag;           // substep whose forward kinematics wave 0 has finished (the other waves' broadphase of the robot boxes waits for it)
  int eoff[NF + NL + 1], efill[NF + NL];
  int wsum[16];
  // contacts: geometry in LDS for the whole solve
  alignas(16) float cp[3][MAXC], cn[3][MAXC];
  // (before the narrowphase has produced them, cp / cn hold the list of candidate BOX pairs and the body pairs' offsets into it: S_SP0 ...)
  // three rows that are, in turn: the narrowphase's staging of (separation, body ids) + the candidate body-pair list; L^-1 of the mass
  // matrix; the unsorted CSR fill order during the solver set-up; and the per-contact impulse P of the current iteration
  float P[3][MAXC];
  unsigned short ent[2 * MAXC];   // CSR entries: contact index | side << 15, grouped by body (bricks, then links), ascending contact index
  float lmf[NL];        // k_physics<.. | SDX_PHYS_DR> only: this env's link mass (and inertia) factors (last: nothing above moves)
};
// Who owns the aliased rows when (one substep, left to right; "-" = dead, anybody may take it).  Each row is MAXC words.
//
// region | mass matrix (B)       | broadphase mask         | collide (D)                               | solver set-up                                | solver loop       | between substeps
// -------+-----------------------+-------------------------+-------------------------------------------+----------------------------------------------+-------------------+-----------------------
// P[0]   | S_T: L^-1 [ND][HP]    | -                       | per contact: box-pair word | samples, then | separation read; S_ENT2; then W (all of P)   | impulse P.x       | -
//        |                       |                         | its separation                            |                                              |                   |
// P[1]   | rows of L (Cholesky)  | -                       | per contact: its key, then body a | b << 8| body ids read; S_EBODY2; then W              | impulse P.y       | -
// P[2]   | -                     | -                       | S_PAIRS: candidate body pairs             | old warm-start keys; S_LANEMAP; then W       | impulse P.z       | -
// cp     | S_BMASK (part 1 is set| S_BMASK: NT words of    | S_BMASK read at entry; S_SP0 in cp[0..1]; | contact points                               | contact points    | S_BMASK, zeroed by
//        | beside the Cholesky)  | cp[0], set by atomicOr  | then the contact points                   |                                              |                   | k_physics after F
// cn     | -                     | -                       | S_SP1 in cn[0..1], S_OFF in cn[2]; then   | contact normals                              | contact normals   | -
//        |                       |                         | the contact normals                       |                                              |                   |
// ent    | -                     | -                       | S_CKEY: identity of contact c             | S_CKEY read at entry; then the sorted CSR    | CSR entries       | -
//
// W: the link-inertia stages of the set-up (T, U, Lam, path dofs: link_inertia() in sdx_phys_solve.h) run through all three P rows once the CSR fill list is dead.
// The contact rows are dead between the solve and the next substep's collide: that is when waves 1.. set the bits of S_BMASK.
#define S_T(S) (reinterpret_cast<float (*)[HP]>(&(S).P[0][0]))                       // L^-1 (mass matrix phase)
#define S_PAIRS(S) (reinterpret_cast<uint32_t*>(&(S).P[2][0]))                       // candidate body pairs (collide)
#define MAXSP (2 * MAXC)                                                             // candidate box pairs per env
#define S_SP0(S) (reinterpret_cast<uint32_t*>(&(S).cp[0][0]))                        // box pair: box a | sub a << 7 | box b << 11 | sub b << 19
#define S_SP1(S) (reinterpret_cast<uint32_t*>(&(S).cn[0][0]))                        // ... its identity: rank of the body pair << 9 | index of the box pair inside it
#define S_OFF(S) (reinterpret_cast<int*>(&(S).cn[0][0]) + MAXSP)                     // body pair -> first candidate box pair (exclusive prefix sum)
#define S_BMASK(S) (reinterpret_cast<uint32_t*>(&(S).cp[0][0]))                       // broadphase hits of lane tid's candidates (bit = trip), NT words; zero between substeps
#define S_LANEMAP(S) (reinterpret_cast<unsigned short*>(&(S).P[2][0]))                // solver set-up: lane -> (brick, lane of the brick) of the balanced gather, [NT]
#define S_ENT2(S) (reinterpret_cast<unsigned short*>(&(S).P[0][0]))                  // unsorted CSR entries (solver set-up)
#define S_EBODY2(S) (reinterpret_cast<unsigned char*>(&(S).P[1][0]))                 // ... and the body each one belongs to
#define S_CKEY(S) (reinterpret_cast<uint32_t*>(&(S).ent[0]))   // identity of contact c until the solver's set-up has read it (the CSR lives here later)
static_assert(ND * HP <= MAXC, "L^-1 must fit one row");
static_assert(MAXP <= MAXC, "the pair list must fit one row");
static_assert(MAXSP + MAXP + 1 <= 3 * MAXC, "box pairs and body-pair offsets fit the rows of cn");
static_assert(3 * 8 * 33 < 1024, "box-pair counts of three body pairs per lane in 10 bits");
static_assert(2 * MAXC * sizeof(unsigned short) == MAXC * sizeof(uint32_t), "contact keys alias the CSR entries");
static_assert(sizeof(PhysLds) <= 80 * 1024, "two workgroups per CU need <= 80 KiB of LDS each");
// The randomization variant (k_physics<512 | SDX_PHYS_DR>) uses the same layout: PhysLds leaves ~50 bytes of the 80 KiB besides lmf, too few
// for this env's other parameter rows (include/seqdex.h SDX_T_DR_*), which are read from HBM where they are used - once per step or
// substep per DOF, once per solve per contact (friction): no access inside the solver's iteration loop

struct Box { f3 c; f4 q; f3 h; };
// phase clock of env B.dbg_env (tools/time_physics.py): compiled in only with -DSDX_PHASE_CLOCK (make prof -> lib/libseqdex_prof.so, selected
// with SDX_LIB_PATH); the stamps keep a zero VGPR and the debug pointer alive through the whole kernel, which the production build does not pay for
#ifdef SDX_PHASE_CLOCK
#define PSTAMP(i) do { if (threadIdx.x == 0 && e == B.dbg_env && sub == 0) B.dbg[i] = (long long)__builtin_readcyclecounter(); } while (0)
#define SSTAMP(i) do { if (threadIdx.x == 0 && dbg) dbg[i] = (long long)__builtin_readcyclecounter(); } while (0)
#define SCOUNT(i, v) do { if (threadIdx.x == 0 && dbg) dbg[i] = (long long)(v); } while (0)
// per-lane measurements of the first solver pass of the debug env: maximum over the block's lanes (slots 55..62 hold maxima since sdx_create)
#ifdef SDX_LANE_CLOCK   // (its global atomics distort the phase stamps of the passes they measure: a build of its own, make prof VFLAGS=-DSDX_LANE_CLOCK)
#define LCLOCK(var) const long long var = (long long)__builtin_readcyclecounter()
#define LMAX(i, v) do { if (dbg) atomicMax(reinterpret_cast<unsigned long long*>(&dbg[i]), (unsigned long long)(v)); } while (0)
#else
#define LCLOCK(var) ((void)0)
#define LMAX(i, v) ((void)0)
#endif
// timing ablations of the profiling build (tools/ablate_physics.py): bits of SDX_T_DEBUG[63], read once per workgroup.  A set bit REMOVES a
// piece of work (the results are then meaningless; the tool restores the state before every launch): 1 the gather loop of [D], 2 the body of
// [AC], 4 all solver iterations but one, 8 the robot section, 16 the sample classification (no contacts), 32 the broadphase (no pairs),
// 64 the solver set-up's rank pass, 128 the row weights, 256 FK + drive of the second substep, 512 the mass matrix
#define ABL(bit) (abl_bits & (bit))
#else
#define PSTAMP(i) ((void)0)
#define SSTAMP(i) ((void)0)
#define SCOUNT(i, v) ((void)0)
#define LCLOCK(var) ((void)0)
#define LMAX(i, v) ((void)0)
#define ABL(bit) 0
#endif
