// stac_planner.hip -- plan construction of libstac_hip.so: builds the "plan" (marker-ancestor subtree, level schedule, CSR site /
// child lists, the kinematics and wrench-sum programs) from the flat model tables, and the shape arithmetic the launches are sized
// with.  Pure host code: NOTHING in this file calls the HIP runtime (the model's device side: stac_model.hip; launches: stac_q.hip).
#include <cmath>
#include <cstdio>

#include "stac_host.hpp"

// The packed tables of fk_kernel (stac_kernels.hip; layout: FullModel in stac_plan.hpp).  A lane carries the transform of the
// body it has just computed in registers; a body whose children do not ALL follow it directly parks its transform in an LDS slot
// until its last child has read it.  Slots are handed out like registers: a slot is free again from the step of its owner's
// last child on (that step reads before it writes).
FkTables build_fk_tables(const stac_model_tables *t) {
    const int nb = t->nbody, nj = t->njnt, K = t->nsite;
    FkTables ft;
    ft.brec.assign((size_t)16 * std::max(nb, 1), 0);
    ft.jrec.assign((size_t)12 * std::max(nj, 1), 0);
    auto f2i = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return i; };
    std::vector<int> last_child(nb, -1), slot_of(nb, -1), owner;  // owner[slot] = body parked there
    std::vector<char> far_child(nb, 0);
    for (int b = 1; b < nb; ++b) {
        const int p = t->body_parentid[b];
        last_child[p] = b;
        if (p != b - 1) far_child[p] = 1;
    }
    for (int b = 0; b < nb; ++b) {
        int32_t *r = &ft.brec[(size_t)16 * b];
        const int p = b ? t->body_parentid[b] : -1;
        r[0] = (b && p != b - 1) ? slot_of[p] : -1;
        r[1] = -1;
        if (far_child[b]) {
            int sl = -1;
            for (int k = 0; k < (int)owner.size() && sl < 0; ++k)
                if (last_child[owner[k]] <= b) sl = k;
            if (sl < 0) { sl = (int)owner.size(); owner.push_back(b); }
            owner[sl] = b;
            slot_of[b] = sl;
            r[1] = sl;
        }
        r[2] = t->body_jntadr[b] < 0 ? 0 : t->body_jntadr[b];
        r[3] = t->body_jntnum[b];
        for (int c = 0; c < 3; ++c) r[4 + c] = f2i(t->body_pos[3 * b + c]);
        for (int c = 0; c < 4; ++c) r[8 + c] = f2i(t->body_quat[4 * b + c]);
        r[7] = (int32_t)ft.sites.size();
        for (int k = 0; k < K; ++k)
            if (t->site_bodyid[k] == b) ft.sites.push_back(k);
        r[12] = (int32_t)ft.sites.size();
    }
    ft.nslots = (int)owner.size();
    for (int j = 0; j < nj; ++j) {
        int32_t *r = &ft.jrec[(size_t)12 * j];
        r[0] = t->jnt_type[j];
        r[1] = t->jnt_qposadr[j];
        r[2] = f2i(t->qpos0[t->jnt_qposadr[j]]);
        r[3] = t->jnt_qposadr[j];
        for (int c = 0; c < 3; ++c) { r[4 + c] = f2i(t->jnt_pos[3 * j + c]); r[8 + c] = f2i(t->jnt_axis[3 * j + c]); }
    }
    // the kernel requests the first coordinate of the joint it will visit TWO steps on while it works on the current one: the order
    // of the visits is the bodies' (body 0 has none); brec[13], brec[14] of body 0 = the coordinates of the first two joints visited
    std::vector<int> visit;
    for (int b = 1; b < nb; ++b)
        for (int j = t->body_jntadr[b]; j < t->body_jntadr[b] + t->body_jntnum[b]; ++j) visit.push_back(j);
    for (size_t i = 0; i < visit.size(); ++i) {
        if (i < 2) ft.brec[13 + i] = t->jnt_qposadr[visit[i]];
        if (i + 2 < visit.size()) ft.jrec[(size_t)12 * visit[i] + 3] = t->jnt_qposadr[visit[i + 2]];
    }
    if (ft.sites.empty()) ft.sites.push_back(0);
    return ft;
}

// The FK program of the bodies in `need` (null: all active bodies): a header (one FK_ML_* flag word per micro-level,
// then per position the ql offset of its first step) and the FkStep records at (micro_level * max_width + position in
// the level).  Positions are those of the full layout, so a child still follows its parent on one lane.
std::vector<int32_t> build_fk_program(const stac_model *m, const char *need, int *n_mlev_out, int *uniform_out, int ja_keep, int *n_run_out) {
    const PlanHeader &h = m->h;
    const int W = h.max_width, rw = h.fk_rec_words, nlev = h.nlev, hw = h.fk_hdr_words;
    const std::vector<int> &lev_adr = m->h_lev_adr;
    // Start step of every body: as soon as its parent is finished and its lane position is free (positions are those of
    // the level layout, so a position runs its bodies in level order and a child that takes over its parent's position
    // starts in the step after the parent's last).  A level no longer waits for its slowest body.
    std::vector<int> tstart(m->h_brec.size(), 0), tfin(m->h_brec.size(), 0), free_t(W, 0);
    int t_end = 0;
    for (int l = 0; l < nlev; ++l)
        for (int s = lev_adr[l]; s < lev_adr[l + 1]; ++s) {
            if (need && !need[s]) continue;
            const int pp = s - lev_adr[l], ps = m->h_ab_parent[s];  // parent slot + 1, 0 = world
            tstart[s] = std::max(ps ? tfin[ps - 1] : 0, free_t[pp]);
            tfin[s] = tstart[s] + std::max(1, m->h_ab_jnum[s]);
            free_t[pp] = tfin[s];
            t_end = std::max(t_end, tfin[s]);
        }
    const int n_mlev = std::max((t_end + 1) & ~1, 2);  // even: the kernel runs two steps per loop trip
    auto f2i = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return i; };
    const int32_t ident_ql = h.c_bx + kXq;  // the world entry's quaternion (1, 0, 0, 0)
    std::vector<int32_t> prog((size_t)hw + (size_t)n_mlev * W * rw, 0);
    for (int ml = 0; ml < n_mlev; ++ml)
        for (int pp = 0; pp < W; ++pp) {  // a position without work: neutral data, nothing stored
            int32_t *r = prog.data() + hw + ((size_t)ml * W + pp) * rw;
            r[4] = -1; r[5] = h.c_sink; r[6] = h.c_sink; r[7] = ident_ql; r[3] = FK_KIND_PLAIN;
            if (rw == 16) r[12] = f2i(1.0f);
        }
    std::vector<int32_t> ql_of((size_t)n_mlev * W, ident_ql);  // ql offset of every (micro-level, position)
    for (int l = 0; l < nlev; ++l)
        for (int s = lev_adr[l]; s < lev_adr[l + 1]; ++s) {
            if (need && !need[s]) continue;
            const BodyRec &br = m->h_brec[s];
            const int pp = s - lev_adr[l], njs = m->h_ab_jnum[s], nsteps = std::max(1, njs), xfs = m->h_xf[s];
            for (int i = 0; i < nsteps; ++i) {
                const int ml = tstart[s] + i;
                int32_t *r = prog.data() + hw + ((size_t)ml * W + pp) * rw;
                const int fsh = 16 * (ml & 1);
                if (i == 0) {
                    prog[ml >> 1] |= FK_ML_BODY << fsh;
                    if (!(br.flags & 1)) prog[ml >> 1] |= FK_ML_BQUAT << fsh;
                    if (!(br.flags & 2)) {  // the parent's transform comes from LDS (another lane produced it, or the world)
                        r[4] = h.c_bx + kXf * br.parent;
                        prog[ml >> 1] |= FK_ML_PARENT_LDS << fsh;
                    }
                    for (int c = 0; c < 3; ++c) r[c] = f2i(br.pos[c]);
                    if (rw == 16) for (int c = 0; c < 4; ++c) r[12 + c] = f2i(br.quat[c]);
                }
                if (i < njs) {
                    const int j = m->h_ab_jadr[s] + i, ty = m->h_aj_type[j];
                    const float *jp = m->h_aj_pos.data() + 3 * j;
                    for (int c = 0; c < 3; ++c) r[8 + c] = f2i(jp[c]);
                    r[5] = j < ja_keep ? h.c_ja + kXf * j : h.c_sink;
                    const bool free_as_parent = ty == STAC_JNT_FREE && i == 0 && br.parent == 0 && (br.flags & 1);
                    if (!free_as_parent) {
                        ql_of[(size_t)ml * W + pp] = h.c_ja + kXf * j + kXq;
                        prog[ml >> 1] |= FK_ML_JOINT << fsh;
                        if (jp[0] != 0.0f || jp[1] != 0.0f || jp[2] != 0.0f) prog[ml >> 1] |= FK_ML_JPOS << fsh;
                    }
                    if (free_as_parent) {
                        // A free joint on a top-level body without orientation is a plain step on a synthetic parent: the
                        // pre-pass leaves {qpos[0:3], normalised quaternion} in the joint's own entry, and with body_pos = 0,
                        // an identity joint quaternion and jnt_pos = 0 the step reproduces exactly that transform
                        // (anchor = position; the free joint's gradient does not look at the pre-joint quaternion).
                        r[4] = h.c_ja + kXf * j;
                        prog[ml >> 1] |= FK_ML_PARENT_LDS << fsh;
                        for (int c = 0; c < 3; ++c) { r[c] = 0; r[8 + c] = 0; }
                    } else if (ty == STAC_JNT_FREE) { r[3] = FK_KIND_FREE; r[11] = m->h_aj_qadr[j]; prog[ml >> 1] |= FK_ML_SPECIAL << fsh; }
                    if (ty == STAC_JNT_SLIDE) { r[3] = FK_KIND_SLIDE; r[11] = j; prog[ml >> 1] |= (FK_ML_SPECIAL | FK_ML_JPOS) << fsh; }
                }
                if (i == nsteps - 1 && xfs >= 0) r[6] = h.c_bx + kXf * xfs;
            }
        }
    for (int ml = 0; ml + 1 < n_mlev; ++ml)
        for (int pp = 0; pp < W; ++pp) prog[hw + ((size_t)ml * W + pp) * rw + 7] = ql_of[(size_t)(ml + 1) * W + pp];
    for (int pp = 0; pp < W; ++pp) prog[(h.n_mlev_hdr >> 1) + pp] = ql_of[pp];  // first steps: fetched by the prologue
    bool uniform = true;
    for (int ml = 0; ml < n_mlev; ++ml) {  // step form (FK_FORM_*) next to the flags
        const int fsh = 16 * (ml & 1), fl = (prog[ml >> 1] >> fsh) & 255;
        // hinge / ball steps on neutral data where a part does not apply (body_pos = 0, jnt_pos = 0, identity joint
        // quaternion: exact no-ops; a position without a joint stores to the sink); free and slide joints and oriented
        // bodies take the general step
        int form = FK_FORM_GENERAL;
        if (!(fl & (FK_ML_SPECIAL | FK_ML_BQUAT))) form = (fl & FK_ML_PARENT_LDS) ? FK_FORM_PARENT_BODY_JOINT : FK_FORM_BODY_JOINT;
        if (form == FK_FORM_GENERAL) uniform = false;
        prog[ml >> 1] |= form << (fsh + 8);
    }
    if (m->dbg.verbose) {
        fprintf(stderr, "[stac] FK program%s: %d steps, forms", need ? " (root passes)" : "", n_mlev);
        for (int ml = 0; ml < n_mlev; ++ml) fprintf(stderr, " %d(%x)", (prog[ml >> 1] >> (16 * (ml & 1) + 8)) & 255, (prog[ml >> 1] >> (16 * (ml & 1))) & 255);
        fprintf(stderr, "\n");
    }
    *n_mlev_out = n_mlev;
    if (n_run_out) *n_run_out = std::max(t_end, 1);  // steps with work (the records are padded to an even count)
    if (uniform_out) *uniform_out = uniform ? 1 : 0;
    return prog;
}

// ---- split kinematics (PlanHeader::fk3): the three tables of a program ---------------------------------------------------------
// P1 runs one quaternion product per active hinge, P3 one addition per rotation that is not identically zero; both are list-
// scheduled (longest remaining path first) on four lane positions.  A position continues with the successor of its last
// operation where there is one -- the running value stays in its registers --, any other operation "restarts" from the LDS
// entry of its predecessor.  Returns false if the program does not fit (more than 32 steps, offsets beyond 16 bits).
struct Fk3Op { int prev; int height; int t = -1, pp = -1; bool restart = false; };
// B, D: an operation may restart only in a step t with t % B == 0, and only from a predecessor finished in a step <= t - D (the
// kernel requests the restart value that far ahead: fk3_p3); a restart from the root position (prev < 0) is always possible.
static int fk3_schedule(std::vector<Fk3Op> &ops, const int B, const int D) {  // returns the number of steps
    const int n = (int)ops.size(), W = 4;
    for (int i = 0; i < n; ++i) ops[i].height = 1;
    for (bool changed = true; changed;) {  // (copies made by fk3_unshare stand behind their successors: no index order to rely on)
        changed = false;
        for (int i = 0; i < n; ++i) {
            const int p = ops[i].prev;
            if (p >= 0 && ops[p].height < ops[i].height + 1) { ops[p].height = ops[i].height + 1; changed = true; }
        }
    }
    std::vector<int> last(W, -2);  // last operation of every position (-2: none yet)
    int done = 0, t = 0;
    for (; done < n; ++t) {
        std::vector<char> taken(W, 0);
        for (int pp = 0; pp < W; ++pp) {  // continue where a successor exists
            if (last[pp] < 0) continue;
            int best = -1;
            for (int i = 0; i < n; ++i)
                if (ops[i].t < 0 && ops[i].prev == last[pp] && (best < 0 || ops[i].height > ops[best].height)) best = i;
            if (best >= 0) { ops[best].t = t; ops[best].pp = pp; taken[pp] = 1; last[pp] = best; ++done; }
        }
        for (int pp = 0; pp < W && t % B == 0; ++pp) {  // free positions take the most urgent operation whose predecessor is finished
            if (taken[pp]) continue;
            int best = -1;
            for (int i = 0; i < n; ++i)
                if (ops[i].t < 0 && (ops[i].prev < 0 || (ops[ops[i].prev].t >= 0 && ops[ops[i].prev].t <= t - D)) &&
                    (best < 0 || ops[i].height > ops[best].height))
                    best = i;
            if (best >= 0) { ops[best].t = t; ops[best].pp = pp; ops[best].restart = true; taken[pp] = 1; last[pp] = best; ++done; }
        }
        if (t > 4 * n + 8) return -1;
    }
    return t;
}
// A restart waits for its source (fk3_schedule: D steps, then the next block), so a branch close to the root would hold its whole
// subtree back.  An operation at depth <= L with several successors therefore gives every successor but the highest its own copy of
// the chain from the root (same operands, same order: the same bits, computed once more by a position that would idle anyway).
// copy(i) appends a copy of operation i's payload and is called once per copied operation, in chain order.
template <class Copy>
static void fk3_unshare(std::vector<Fk3Op> &ops, const int L, Copy &&copy) {
    const int n = (int)ops.size();
    std::vector<int> depth(n, 0), height(n, 1);
    for (int i = 0; i < n; ++i) depth[i] = (ops[i].prev >= 0 ? depth[ops[i].prev] : 0) + 1;  // (prev < i here)
    for (int i = n - 1; i >= 0; --i)
        if (ops[i].prev >= 0) height[ops[i].prev] = std::max(height[ops[i].prev], height[i] + 1);
    for (int i = 0; i < n; ++i) {
        if (depth[i] > L) continue;
        std::vector<int> kids;
        for (int k = i + 1; k < n; ++k)
            if (ops[k].prev == i) kids.push_back(k);
        if (kids.size() < 2) continue;
        std::stable_sort(kids.begin(), kids.end(), [&](int x, int y) { return height[x] > height[y]; });
        std::vector<int> chain;
        for (int j = i; j >= 0; j = ops[j].prev) chain.push_back(j);
        for (size_t c = 1; c < kids.size(); ++c) {
            int last = -1;
            for (int q = (int)chain.size() - 1; q >= 0; --q) {
                ops.push_back(Fk3Op{last, 0});
                copy(chain[q]);
                last = (int)ops.size() - 1;
            }
            ops[kids[c]].prev = last;
        }
    }
}
bool build_fk3_program(const stac_model *m, const PlanHeader &h3, const char *need, int cap1, int cap2, int cap3, Fk3Program &out) {
    const int nab = h3.nab, naj = h3.naj, K = h3.K;
    auto f2i = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return i; };
    auto nz3 = [](const float *v) { return v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f; };
    // Quaternion nodes (entries of the chain's c3_qb array): node j = the quaternion AFTER active joint j (node 0: the free root's, from the
    // pre-pass), node naj = the sink of idle positions, node naj + 1 + i = the quaternion of the i-th ORIENTED body (body_quat not the
    // identity, below the root body) before its joints: q_parent * body_quat, the oracle's own order (oracle/stac_oracle.c: fk_chain).
    // fin[s]: node of body s after its last joint (else its oriented-body node, else its parent's); pre[j]: node in front of joint j.
    std::vector<int> fin(nab, 0), pre(naj, 0), bnode(nab, -1), bpre(nab, 0);
    int nbq = 0;
    for (int s = 0; s < nab; ++s) {
        const int ps = m->h_ab_parent[s] - 1;
        int cur = ps >= 0 ? fin[ps] : 0;
        if (s != 0 && !(m->h_brec[s].flags & 1)) { bpre[s] = cur; bnode[s] = naj + 1 + nbq; cur = bnode[s]; ++nbq; }
        for (int i = 0; i < m->h_ab_jnum[s]; ++i) { const int j = m->h_ab_jadr[s] + i; pre[j] = cur; cur = j; }
        fin[s] = cur;
    }
    if (nbq != h3.nbq) return false;  // (the layout was made for the model's own count: build_plan)
    // P1: one product per needed hinge, and one per needed oriented body (its factor: the constant body_quat, which every chain region
    // holds in c3_bq -- written once per launch, q_phase_kernel's prologue)
    struct Prod { int qlw, node, prenode; };  // word of the right factor, node of the result, node of the left factor
    std::vector<Fk3Op> o1;
    std::vector<Prod> p_of1;
    std::vector<int> op_of_node(naj + 1 + nbq, -1);
    for (int s = 0; s < nab; ++s) {
        if (need && !need[s]) continue;
        if (bnode[s] >= 0) {
            op_of_node[bnode[s]] = (int)o1.size();
            o1.push_back(Fk3Op{bpre[s] == 0 ? -1 : op_of_node[bpre[s]], 0});
            p_of1.push_back(Prod{h3.c3_bq + 4 * (bnode[s] - naj - 1), bnode[s], bpre[s]});
        }
        for (int i = 0; i < m->h_ab_jnum[s]; ++i) {
            const int j = m->h_ab_jadr[s] + i;
            if (j == 0) continue;  // the free root: its quaternion comes from the pre-pass
            op_of_node[j] = (int)o1.size();
            o1.push_back(Fk3Op{pre[j] == 0 ? -1 : op_of_node[pre[j]], 0});
            p_of1.push_back(Prod{h3.c3_ql + 4 * j, j, pre[j]});
        }
    }
    // P3: the additions, in the order of the step program (body_pos, then per joint anchor and position)
    struct Rot { int qnode; float v[3]; };
    std::vector<Fk3Op> o3;
    std::vector<Rot> rot;  // one per P3 operation
    std::vector<int> body_op(nab, -1), anchor_op(naj, -1);
    for (int s = 0; s < nab; ++s) {
        if (need && !need[s]) continue;
        const int ps = m->h_ab_parent[s] - 1;
        int cur = ps >= 0 ? body_op[ps] : -1;
        const float *bp = m->h_bpos.data() + 3 * s;
        if (s != 0 && nz3(bp)) {
            o3.push_back(Fk3Op{cur, 0});
            rot.push_back(Rot{ps >= 0 ? fin[ps] : 0, {bp[0], bp[1], bp[2]}});
            cur = (int)o3.size() - 1;
        }
        for (int i = 0; i < m->h_ab_jnum[s]; ++i) {
            const int j = m->h_ab_jadr[s] + i;
            if (j == 0) { cur = -1; anchor_op[j] = -1; continue; }  // free root: position = qpos[0:3]
            const float *jp = m->h_aj_pos.data() + 3 * j;
            if (nz3(jp)) {
                o3.push_back(Fk3Op{cur, 0});
                rot.push_back(Rot{pre[j], {jp[0], jp[1], jp[2]}});        // anchor = rotate(jpos, prequat) + pos
                cur = (int)o3.size() - 1;
                anchor_op[j] = cur;
                o3.push_back(Fk3Op{cur, 0});
                rot.push_back(Rot{j, {-jp[0], -jp[1], -jp[2]}});          // pos = anchor - rotate(jpos, quat): rotate is odd in v
                cur = (int)o3.size() - 1;
            } else {
                anchor_op[j] = cur;
            }
        }
        body_op[s] = cur;
    }
    fk3_unshare(o1, 2, [&](int i) { p_of1.push_back(p_of1[i]); });
    fk3_unshare(o3, 4, [&](int i) { rot.push_back(rot[i]); });
    int n1 = fk3_schedule(o1, 2, 3);
    if (n1 > 0) n1 = (n1 + 1) & ~1;  // P1 runs whole blocks of two steps
    int n3 = fk3_schedule(o3, 4, 5);
    if (n3 > 0) n3 = (n3 + 3) & ~3;  // P3 runs whole blocks of four steps
    const int n2 = ((int)o3.size() + 15) & ~15;  // P2 runs whole rounds of 16 lanes (32-lane groups: the area's no-ops behind them, cap2)
    if (n1 < 0 || n3 < 0 || n1 > 254 || n3 > 252 || n1 > cap1 || n3 > cap3 || n2 > cap2) return false;  // (eight bits each in PlanHeader::fk3_n)
    const int root_slot = cap3 * 4, sink_slot = cap3 * 4 + 1;
    auto pbw = [&](int op) { return h3.c3_pb + 3 * (op < 0 ? root_slot : o3[op].t * 4 + o3[op].pp); };
    auto qbw = [&](int node) { return h3.c3_qb + 4 * node; };
    if (h3.stride3 >= 65536) return false;
    out.n1 = std::max(n1, 0); out.n2 = n2; out.n3 = n3; out.nrot = (int)o3.size();
    // T1, blocks of two steps, 24 words per record: [24 r + 4 pp] = {ql word of step 2 r, of step 2 r + 1, out word of step 2 r - 2, of
    // 2 r - 1}, [24 r + 16 + 2 pp] = {restart entry of block r - 1, of block r} -- record r + 1 is what block r works from (its out words,
    // its restart flag, the next block's ql and restart words), record 0 the prologue.  A restart entry: the word of the quaternion the
    // position starts the block from, or bit 31 | a valid word if it keeps its running value.  cap1 / 2 + 3 records (P1 fetches one
    // record ahead and runs pairs of blocks); an idle step multiplies by any quaternion into the sink.
    out.words.assign((size_t)16 * (cap1 + 2) + 4 * (size_t)cap2 + 4 * (size_t)cap3 + K + naj, 0);
    int32_t *T1 = out.words.data(), *T2 = T1 + 16 * (cap1 + 2), *T3 = T2 + 4 * cap2, *SW = T3 + 4 * cap3, *JW = SW + K;
    const int nrec1 = cap1 / 2 + 3;
    if (24 * nrec1 > 16 * (cap1 + 2)) return false;  // (cap1 >= 10: build_plan)
    for (int r = 0; r < nrec1; ++r)
        for (int pp = 0; pp < 4; ++pp) {
            int32_t *w = T1 + 24 * r + 4 * pp, *e = T1 + 24 * r + 16 + 2 * pp;
            w[0] = w[1] = h3.c3_ql; w[2] = w[3] = qbw(naj);
            e[0] = e[1] = (int32_t)(0x80000000u | (uint32_t)qbw(0));
        }
    for (size_t i = 0; i < o1.size(); ++i) {
        const Prod &pr = p_of1[i];
        const int blk = o1[i].t >> 1, k = o1[i].t & 1, pp = o1[i].pp;
        T1[24 * blk + 4 * pp + k] = pr.qlw;
        T1[24 * (blk + 1) + 4 * pp + 2 + k] = qbw(pr.node);
        if (o1[i].restart) {  // (only in the first step of a block: fk3_schedule)
            T1[24 * blk + 16 + 2 * pp + 1] = qbw(pr.prenode);
            T1[24 * (blk + 1) + 16 + 2 * pp] = qbw(pr.prenode);
        }
    }
    for (int i = 0; i < cap2; ++i) { T2[4 * i + 3] = qbw(0) | (h3.c3_pb + 3 * sink_slot) << 16; }  // no-op: rotate(0, root quaternion) into the sink
    for (size_t i = 0; i < o3.size(); ++i) {
        int32_t *r = T2 + 4 * i;
        for (int c = 0; c < 3; ++c) r[c] = f2i(rot[i].v[c]);
        r[3] = qbw(rot[i].qnode) | pbw((int)i) << 16;
    }
    // T3[4 b + pp]: what position pp starts block b (steps 4 b .. 4 b + 3) from -- the word of a restart value, or bit 31 | any valid
    // word if it keeps its running value; cap3 / 4 + 3 blocks (P3 requests three blocks ahead) in the table's 4 cap3 words
    for (int i = 0; i < 4 * cap3; ++i) T3[i] = (int32_t)(0x80000000u | (uint32_t)pbw(-1));
    for (size_t i = 0; i < o3.size(); ++i)
        if (o3[i].restart) T3[o3[i].t + o3[i].pp] = pbw(o3[i].prev);  // (t % 4 == 0: entry 4 (t / 4) + pp)
    for (int k = 0; k < K; ++k) {
        const int sl = m->h_site_slot[k];
        if (need && !need[sl]) { SW[k] = pbw(-1) | qbw(0) << 16; continue; }  // (a site the root passes do not weigh: any valid entry)
        SW[k] = pbw(body_op[sl]) | qbw(fin[sl]) << 16;
    }
    // per joint: word of its anchor | word of its pre-joint quaternion << 16 (the gradient pass; full program only)
    for (int j = 0; j < naj; ++j) JW[j] = need ? 0 : (pbw(anchor_op[j]) | qbw(pre[j]) << 16);
    if (m->dbg.verbose)
        fprintf(stderr, "[stac] FK3 program%s: %d products in %d steps, %d rotations, %d additions in %d steps\n", need ? " (root passes)" : "",
                (int)o1.size(), n1, (int)o3.size(), (int)o3.size(), n3);
    return true;
}

// ------------------------------------------------------------------------------------------------
// plan construction
// ------------------------------------------------------------------------------------------------
static WsumProgram build_wsum_program(const std::vector<RangeRec> &ranges, int K, int parts, int ntask_fixed) {
    const int nr = (int)ranges.size();
    auto len = [&](int r) { return ranges[r].hi - ranges[r].lo; };
    // Cost of a choice, in instructions of the wavefront, with a dependent LDS round trip counted as twelve (a heuristic, from the
    // instruction counts and phase times of profiles/r10/wrench_sums.md).  A round of lanes is as long as its longest loop, and runs the
    // remainder block if any of its lanes has a remainder.  Component tasks: 47 + 25 per trip of four sites + 27 for the remainder; a
    // checkpoint adds the store and a second pair of loops.  Whole ranges: 42 + 62 per trip + 72.  Sweeps, per row: the record, the
    // entry and A_0 (11), six additions per further step, five instructions per step for the stores, two round trips.
    auto round_cost = [&](const std::vector<int> &lens, bool task, bool ckpt) {
        int trips = 0;
        bool rem = false;
        for (const int n : lens) { trips = std::max(trips, n / 4); rem = rem || (n % 4) != 0; }
        return task ? 47.0 + 25.0 * trips + (rem ? 27.0 : 0.0) + (ckpt ? 10.0 : 0.0) : 42.0 + 62.0 * trips + (rem ? 72.0 : 0.0);
    };
    WsumProgram best;
    bool have = false;
    const int max_depth = (parts & 1) && nr < kWsumNone ? kWsumMaxDepth : 0;
    for (int depth = 0; depth <= max_depth; ++depth) {
        // rows: as few as hold the sites; with two, the cut may sit wherever both keep to 16 sites
        const int cut_lo = depth == 0 || K <= 16 ? 0 : K - 16, cut_hi = depth == 0 || K <= 16 ? 0 : 16;
        for (int cut = cut_lo; cut <= cut_hi; ++cut) {
            WsumProgram pr;
            pr.depth = depth;
            if (depth > 0) {
                pr.nrows = cut > 0 ? 2 : 1;
                pr.row_start[1] = cut > 0 ? cut : K;
                pr.row_start[2] = K;
            }
            std::vector<char> swept(nr, 0);
            if (depth > 0) {
                pr.rows.assign((size_t)pr.nrows * 32, 0);
                for (int row = 0; row < pr.nrows; ++row)
                    for (int l = 0; l < 16; ++l) {
                        pr.rows[2 * (row * 16 + l)] = kXf * std::min(pr.row_start[row] + l, pr.row_start[row + 1] - 1);
                        pr.rows[2 * (row * 16 + l) + 1] = (int32_t)0xFFFFFFFFu;  // (kWsumNone in every byte)
                    }
                for (int r = 0; r < nr; ++r) {
                    if (len(r) < 1 || len(r) > depth) continue;
                    const int row = (pr.nrows == 2 && ranges[r].lo >= cut) ? 1 : 0;
                    if (ranges[r].hi > pr.row_start[row + 1]) continue;  // crosses the cut: not a sweep's
                    swept[r] = 1;
                    int32_t &cap = pr.rows[2 * (row * 16 + ranges[r].hi - 1 - pr.row_start[row]) + 1];
                    const int sh = 8 * (len(r) - 1);
                    cap = (int32_t)(((uint32_t)cap & ~(0xFFu << sh)) | ((uint32_t)r << sh));
                }
                pr.cost += pr.nrows * (11.0 + 6.0 * (depth - 1) + 5.0 * depth + 24.0);
                bool any_swept = false;
                for (int r = 0; r < nr; ++r) any_swept = any_swept || swept[r];
                if (!any_swept) continue;  // (depth 0 is this program without the rows)
            }
            // what is left, longest first; a range takes the longest shorter one with its first site as its checkpoint
            std::vector<int> rest, ckpt(nr, -1), owner(nr, -1);
            for (int r = 0; r < nr; ++r)
                if (!swept[r]) rest.push_back(r);
            if (parts & 2)
                for (size_t i = 0; i < rest.size(); ++i) {
                    const int r = rest[i];
                    if (owner[r] >= 0) continue;
                    for (size_t j = i + 1; j < rest.size(); ++j) {
                        const int c = rest[j];
                        if (owner[c] < 0 && ckpt[c] < 0 && ranges[c].lo == ranges[r].lo && len(c) >= 1 && len(c) < len(r)) {
                            ckpt[r] = c; owner[c] = r;
                            break;
                        }
                    }
                }
            std::vector<int> units;
            for (const int r : rest)
                if (owner[r] < 0) units.push_back(r);
            const int nu = (int)units.size();
            const int ns_lo = ntask_fixed >= 0 ? std::min(ntask_fixed, nu) : 0, ns_hi = ntask_fixed >= 0 ? ns_lo : nu;
            for (int ns = ns_lo; ns <= ns_hi; ++ns) {
                WsumProgram q = pr;
                q.ntask = ns;
                for (int u = 0; u < ns; ++u) {
                    const int r = units[u], c = ckpt[r];
                    q.recs.push_back(WsumRec{ranges[r].lo, c >= 0 ? ranges[c].hi : ranges[r].hi, ranges[r].hi, (c >= 0 ? c : r) | r << 16});
                }
                std::vector<char> is_task(nr, 0);
                for (int u = 0; u < ns; ++u) { is_task[units[u]] = 1; if (ckpt[units[u]] >= 0) is_task[ckpt[units[u]]] = 1; }
                for (const int r : rest)
                    if (!is_task[r]) { q.recs.push_back(WsumRec{ranges[r].lo, ranges[r].hi, ranges[r].hi, r | r << 16}); ++q.nwhole; }
                for (int t0 = 0; t0 < 6 * ns; t0 += 16) {
                    std::vector<int> lens;
                    bool ck = false;
                    for (int t1 = t0; t1 < std::min(t0 + 16, 6 * ns); ++t1) {
                        const WsumRec &w = q.recs[t1 / 6];
                        lens.push_back(w.mid - w.lo); lens.push_back(w.hi - w.mid);
                        ck = ck || w.mid != w.hi;
                    }
                    // (two loops in series: the trips of both; one remainder block each at the most)
                    std::vector<int> l1, l2;
                    for (size_t i = 0; i < lens.size(); i += 2) { l1.push_back(lens[i]); l2.push_back(lens[i + 1]); }
                    q.cost += round_cost(l1, true, ck) + (ck ? round_cost(l2, true, false) - 47.0 : 0.0);
                }
                for (int r0 = 0; r0 < q.nwhole; r0 += 16) {
                    std::vector<int> lens;
                    for (int r1 = r0; r1 < std::min(r0 + 16, q.nwhole); ++r1) lens.push_back(q.recs[ns + r1].hi - q.recs[ns + r1].lo);
                    q.cost += round_cost(lens, false, false);
                }
                q.cost += q.ntask + q.nwhole;  // (among equals: the cut that fewer short ranges cross)
                if (q.ntask > 255 || q.nwhole > 255) continue;
                if (!have || q.cost < best.cost) { best = q; have = true; }
            }
        }
    }
    return best;
}

int build_plan(stac_model *m, const stac_model_tables *t) {
    const int nb = t->nbody, nj = t->njnt, nq = t->nq, K = t->nsite;
    if (nb < 2 || nq < 1 || K < 1) return fail(STAC_ERR_INVALID, "model needs >= 1 body, qpos and fit site");
    std::vector<int> depth(nb, 0), active(nb, 0);
    for (int b = 1; b < nb; ++b) {
        const int p = t->body_parentid[b];
        if (p < 0 || p >= b) return fail(STAC_ERR_INVALID, "bodies must be in depth-first order (parent id < body id)");
        depth[b] = depth[p] + 1;
    }
    for (int k = 0; k < K; ++k) {
        const int sb = t->site_bodyid[k];
        if (sb < 0 || sb >= nb) return fail(STAC_ERR_INVALID, "site_bodyid out of range");
        for (int b = sb; b > 0 && !active[b]; b = t->body_parentid[b]) active[b] = 1;
    }
    // Active bodies level by level.  Inside a level a body takes its parent's position wherever that position
    // exists in its own level (the kernel lane that finished the parent then continues with the child and
    // keeps the transform in registers); the deepest subtrees choose first, so long limbs stay on one lane.
    std::vector<int> height(nb, 0);
    for (int b = nb - 1; b >= 1; --b)
        if (active[b]) height[t->body_parentid[b]] = std::max(height[t->body_parentid[b]], height[b] + 1);
    int max_depth_active = 0;
    for (int b = 1; b < nb; ++b)
        if (active[b]) max_depth_active = std::max(max_depth_active, depth[b]);
    std::vector<int> slots, pos_in_level(nb, -1);
    for (int d = 1; d <= max_depth_active; ++d) {
        std::vector<int> bodies;
        for (int b = 1; b < nb; ++b)
            if (active[b] && depth[b] == d) bodies.push_back(b);
        std::stable_sort(bodies.begin(), bodies.end(), [&](int a, int b) { return height[a] > height[b]; });
        const int w = (int)bodies.size();
        std::vector<int> at(w, -1);
        std::vector<char> placed(w, 0);
        for (int i = 0; i < w; ++i) {  // deepest first: inherit the parent's position if it is free
            const int pp = pos_in_level[t->body_parentid[bodies[i]]];
            if (pp >= 0 && pp < w && at[pp] < 0) { at[pp] = bodies[i]; placed[i] = 1; }
        }
        int free_pos = 0;
        for (int i = 0; i < w; ++i) {
            if (placed[i]) continue;
            while (at[free_pos] >= 0) ++free_pos;
            at[free_pos] = bodies[i];
        }
        for (int i = 0; i < w; ++i) { pos_in_level[at[i]] = i; slots.push_back(at[i]); }
    }
    const int nab = (int)slots.size();
    if (nab == 0) return fail(STAC_ERR_INVALID, "all fit sites are attached to the world body");
    std::vector<int> slot_of(nb, -1);
    for (int s = 0; s < nab; ++s) slot_of[slots[s]] = s;
    // levels
    std::vector<int> lev_adr;
    for (int s = 0; s < nab; ++s)
        if (s == 0 || depth[slots[s]] != depth[slots[s - 1]]) lev_adr.push_back(s);
    const int nlev = (int)lev_adr.size();
    lev_adr.push_back(nab);
    // contiguous depth levels are required (an active body's parent is active, one level up)
    // joints
    std::vector<int> ab_jadr(nab), ab_jnum(nab), aj_type, aj_qadr, aj_slot;
    std::vector<float> aj_pos, aj_axis, aj_q0;
    int has_ball = 0;
    for (int s = 0; s < nab; ++s) {
        const int b = slots[s];
        ab_jadr[s] = (int)aj_type.size();
        ab_jnum[s] = t->body_jntnum[b];
        for (int j = t->body_jntadr[b]; j < t->body_jntadr[b] + t->body_jntnum[b]; ++j) {
            const int ty = t->jnt_type[j];
            if (ty < 0 || ty > 3) return fail(STAC_ERR_INVALID, "unknown joint type");
            if (ty == STAC_JNT_BALL) has_ball = 1;
            aj_type.push_back(ty);
            aj_qadr.push_back(t->jnt_qposadr[j]);
            aj_slot.push_back(s);
            for (int i = 0; i < 3; ++i) { aj_pos.push_back(t->jnt_pos[3 * j + i]); aj_axis.push_back(t->jnt_axis[3 * j + i]); }
            aj_q0.push_back((ty == STAC_JNT_HINGE || ty == STAC_JNT_SLIDE) ? t->qpos0[t->jnt_qposadr[j]] : 0.0f);
        }
    }
    const int naj = (int)aj_type.size();
    // sites sorted by (body id, site id); per joint the range of sorted positions inside its body's subtree
    std::vector<int> ab_parent(nab), sortpos(K), aj_slo(naj), aj_shi(naj), sorted;
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < K; ++k)
            if (t->site_bodyid[k] == b) { sortpos[k] = (int)sorted.size(); sorted.push_back(k); }
    std::vector<int> sub_end(nb);
    for (int b = 0; b < nb; ++b) sub_end[b] = b;
    for (int b = nb - 1; b >= 1; --b) sub_end[t->body_parentid[b]] = std::max(sub_end[t->body_parentid[b]], sub_end[b]);
    for (int s = 0; s < nab; ++s) {
        const int b = slots[s];
        const int p = t->body_parentid[b];
        ab_parent[s] = p == 0 ? 0 : slot_of[p] + 1;
        int lo = 0;
        while (lo < K && t->site_bodyid[sorted[lo]] < b) ++lo;
        int hi = lo;
        while (hi < K && t->site_bodyid[sorted[hi]] <= sub_end[b]) ++hi;
        for (int j = ab_jadr[s]; j < ab_jadr[s] + ab_jnum[s]; ++j) { aj_slo[j] = lo; aj_shi[j] = hi; }
    }
    // quaternion addresses of the whole model
    std::vector<int> quat_adr;
    for (int j = 0; j < nj; ++j) {
        if (t->jnt_type[j] == STAC_JNT_FREE) quat_adr.push_back(t->jnt_qposadr[j] + 3);
        if (t->jnt_type[j] == STAC_JNT_BALL) quat_adr.push_back(t->jnt_qposadr[j]);
    }

    PlanHeader &h = m->h;
    h.nbody = nb; h.njnt = nj; h.nq = nq; h.K = K;
    h.nab = nab; h.naj = naj; h.nlev = nlev; h.nquat = (int)quat_adr.size();
    h.nqpad = (nq + 3) & ~3;
    h.has_ball = has_ball;
    m->max_depth = nlev;
    h.max_width = 0;
    for (int l = 0; l < nlev; ++l) h.max_width = std::max(h.max_width, lev_adr[l + 1] - lev_adr[l]);
    m->h_ab_parent = ab_parent; m->h_aj_type = aj_type; m->h_aj_qadr = aj_qadr; m->h_aj_slot = aj_slot;
    m->h_aj_slo = aj_slo; m->h_aj_shi = aj_shi; m->h_sortpos = sortpos;
    m->h_site_slot.resize(K);
    for (int k = 0; k < K; ++k) m->h_site_slot[k] = slot_of[t->site_bodyid[k]];
    if (nab >= 65535 || K >= 65535) return fail(STAC_ERR_CAPACITY, "too many bodies / sites");
    if (K > 4096) return fail(STAC_ERR_CAPACITY, "more than 4096 fit sites");

    std::vector<float> &B = m->blob_host;
    B.clear();
    auto align4 = [&]() { while (B.size() & 3) B.push_back(0.f); };
    auto put_raw = [&](const void *src, size_t words) {
        align4();
        int off = (int)B.size();
        B.resize(B.size() + words);
        std::memcpy(B.data() + off, src, words * 4);
        align4();
        return off;
    };
    auto put_fpad = [&](const float *src, int n, int padded) {
        std::vector<float> v(src, src + n);
        v.resize(padded, 0.f);
        return put_raw(v.data(), v.size());
    };
    // Which body transforms go to LDS: those a site or a child on ANOTHER lane reads back (a child at its parent's
    // position continues from the lane's registers).  Levels wider than the narrowest lane group (4) can take
    // several passes per level, where nothing is carried: then every transform is stored.
    int max_width0 = 0;
    for (int l = 0; l < nlev; ++l) max_width0 = std::max(max_width0, lev_adr[l + 1] - lev_adr[l]);
    std::vector<int> stored(nab, max_width0 > 4 ? 1 : 0), xf(nab, -1);
    stored[0] = 1;  // moments are taken about the first active body
    for (int k = 0; k < K; ++k) stored[slot_of[t->site_bodyid[k]]] = 1;
    for (int s = 0; s < nab; ++s) {
        const int b = slots[s], pb = t->body_parentid[b];
        if (pb > 0 && pos_in_level[pb] != pos_in_level[b]) stored[slot_of[pb]] = 1;
    }
    int nst = 0;
    for (int s = 0; s < nab; ++s)
        if (stored[s]) xf[s] = ++nst;  // transform index; 0 = world
    std::vector<BodyRec> brec(nab);
    for (int s = 0; s < nab; ++s) {
        const int b = slots[s];
        BodyRec &r = brec[s];
        const int pb = t->body_parentid[b];
        r.parent = pb == 0 ? 0 : std::max(xf[slot_of[pb]], 0);  // transform index (only read when the parent is stored)
        r.jadr = ab_jadr[s]; r.jnum = ab_jnum[s];
        const float *q = t->body_quat + 4 * b;
        r.flags = (q[0] == 1.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f) ? 1 : 0;
        if (pb > 0 && pos_in_level[pb] == pos_in_level[b]) r.flags |= 2;  // parent transform is in the lane's registers
        r.flags |= (xf[s] < 0 ? 0xFFFF : xf[s]) << 16;                    // where this body's transform is stored
        for (int i = 0; i < 3; ++i) r.pos[i] = t->body_pos[3 * b + i];
        r.jzero = 0;
        for (int jj = 0; jj < ab_jnum[s] && jj < 31; ++jj) {
            const float *jp = aj_pos.data() + 3 * (ab_jadr[s] + jj);
            if (jp[0] == 0.0f && jp[1] == 0.0f && jp[2] == 0.0f) r.jzero |= (1 << jj);
        }
        for (int i = 0; i < 4; ++i) r.quat[i] = q[i];
    }
    // distinct site ranges, longest first (the lanes of a round then run loops of similar length)
    std::vector<RangeRec> ranges;
    std::vector<int> aj_rid(naj, 0);
    {
        std::vector<std::pair<int, int>> uniq;
        for (int j = 0; j < naj; ++j) {
            const std::pair<int, int> r{aj_slo[j], aj_shi[j]};
            if (std::find(uniq.begin(), uniq.end(), r) == uniq.end()) uniq.push_back(r);
        }
        std::stable_sort(uniq.begin(), uniq.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) {
            return a.second - a.first > b.second - b.first;
        });
        for (const auto &r : uniq) ranges.push_back(RangeRec{r.first, r.second});
        for (int j = 0; j < naj; ++j)
            aj_rid[j] = (int)(std::find(uniq.begin(), uniq.end(), std::pair<int, int>{aj_slo[j], aj_shi[j]}) - uniq.begin());
        if (ranges.empty()) ranges.push_back(RangeRec{0, 0});
    }
    h.nrange = (int)ranges.size();
    {   // PlanHeader::rsplit: how many of the longest ranges the 16-lane kernels sum one component per lane.  Cost of a choice, in
        // instructions of the wavefront (every round of lanes is as long as its longest loop): a site of a component task is one read and
        // one addition, of a whole range six of each; a round has a fixed part (its record, the stores, the loop).
        auto cost = [&](int ns) {
            const double c1 = 2.5, c6 = 13.0, fixed = 15.0;
            double c = 0.0;
            for (int t0 = 0; t0 < 6 * ns; t0 += 16) c += fixed + c1 * (ranges[t0 / 6].hi - ranges[t0 / 6].lo);  // (sorted: a round's first task is its longest)
            for (int r0 = ns; r0 < h.nrange; r0 += 16) c += fixed + c6 * (ranges[r0].hi - ranges[r0].lo);
            return c;
        };
        int best = 0;
        for (int ns = 1; ns <= h.nrange; ++ns)
            if (cost(ns) < cost(best)) best = ns;
        h.rsplit = m->dbg.rsplit >= 0 ? std::min(m->dbg.rsplit, h.nrange) : best;
    }
    std::vector<JointRec> jrec(std::max(naj, 1));
    int nqj = 0;
    for (int j = 0; j < naj; ++j) {
        JointRec &r = jrec[j];
        r.type = aj_type[j]; r.qadr = aj_qadr[j]; r.slo = aj_slo[j]; r.shi = aj_shi[j];
        for (int i = 0; i < 3; ++i) { r.pos[i] = aj_pos[3 * j + i]; r.axis[i] = aj_axis[3 * j + i]; }
        r.q0 = aj_q0[j]; r.rid = aj_rid[j];
        if (aj_type[j] == STAC_JNT_FREE || aj_type[j] == STAC_JNT_BALL) {  // no reference angle: the ordinal among the
            const int32_t qi = nqj++;                                       // quaternion joints (saved-quaternion slot)
            std::memcpy(&r.q0, &qi, 4);
        }
    }
    std::vector<SiteRec> srec(K);
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < 3; ++i) srec[k].pos[i] = t->site_pos[3 * k + i];
        srec[k].slot_sortpos = xf[slot_of[t->site_bodyid[k]]] | (sortpos[k] << 16);
    }
    h.off_lev_adr = put_raw(lev_adr.data(), lev_adr.size());
    h.off_body = put_raw(brec.data(), brec.size() * sizeof(BodyRec) / 4);
    {   // The wrench-sum program (WsumRec, stac_plan.hpp) of a model that the lean 16-lane throughput kernels can take: the conditions of
        // the split kinematics below that are known by now, and a 16-lane lean shape that holds the model.  Its table stands in front
        // of the momentum table, so that only a lean throughput launch stages it (plan_q, lean_header).  STAC_HIP_NOWSUM (read at model
        // creation): no sweeps and no checkpoints -- PlanHeader::rsplit's split in the program's form, what the kernels ran before.
        m->off_wsum = 0;
        m->wsum = WsumProgram{};
        bool lean16 = kWsum != 0 && naj >= 1 && aj_type[0] == STAC_JNT_FREE && aj_qadr[0] == 0 && ab_jnum[0] >= 1 && ab_jadr[0] == 0 && nqj == 1 &&
                      !has_ball && !m->dbg.nofk3 && h.nrange < kWsumNone && thr_lean_holds(h, 16);
        for (int j = 1; j < naj && lean16; ++j) lean16 = aj_type[j] == STAC_JNT_HINGE;
        for (int s = 1; s < nab && lean16; ++s) lean16 = ab_parent[s] != 0;
        if (lean16) {
            const int parts = m->dbg.nowsum ? 0 : kWsum;
            m->wsum = build_wsum_program(ranges, K, parts, parts == 0 ? h.rsplit : (m->dbg.rsplit >= 0 ? m->dbg.rsplit : -1));
            const std::vector<int32_t> tab = m->wsum.table(0, 0);  // (the words of the lean layout follow once it is made: below)
            m->off_wsum = put_raw(tab.data(), tab.size());
        }
    }
    {   // momentum table (stac_plan.hpp, kTTab): the kernel's expressions, float32, no contraction (build flags)
        std::vector<float> tt(2 * kTTab);
        float tk = 1.0f;
        for (int k = 0; k < kTTab; ++k) {
            const float tn = 0.5f * (1.0f + std::sqrt(1.0f + 4.0f * tk * tk));
            tt[2 * k] = tn;
            tt[2 * k + 1] = (tk - 1.0f) / tn;
            tk = tn;
        }
        (void)put_raw(tt.data(), tt.size());
    }
    h.off_joint = put_raw(jrec.data(), jrec.size() * sizeof(JointRec) / 4);
    h.off_site = put_raw(srec.data(), srec.size() * sizeof(SiteRec) / 4);
    h.off_range = put_raw(ranges.data(), ranges.size() * sizeof(RangeRec) / 4);
    h.off_lb = put_fpad(t->lb, nq, h.nqpad);
    h.off_ub = put_fpad(t->ub, nq, h.nqpad);
    h.off_qpos0 = put_fpad(t->qpos0, nq, h.nqpad);
    quat_adr.push_back(0);
    h.off_quat_adr = put_raw(quat_adr.data(), quat_adr.size());
    {
        std::vector<int32_t> act(h.nqpad, 0);
        for (int j = 0; j < naj; ++j) {
            const int dims = aj_type[j] == STAC_JNT_FREE ? 7 : (aj_type[j] == STAC_JNT_BALL ? 4 : 1);
            for (int c = 0; c < dims; ++c) act[aj_qadr[j] + c] = 1;
        }
        h.off_active = put_raw(act.data(), act.size());
    }
    h.core_words = (int)B.size();  // what a kernel that walks the levels itself stages in LDS
    // per-chain LDS layout
    int o = 0;
    h.nst = nst;
    h.nqj = nqj;
    h.c_bx = o; o += (nst + 1) * kXf;
    h.c_ja = o; o += naj * kXf;
    h.c_jn = o; o += std::max(nqj, 1);
    h.c_qsv = o; o += 4 * nqj;
    o = (o + 3) & ~3;
    h.c_sw = o; o += std::max(K * kXf, h.nqpad + kXf);  // (+ kXf: the tail entry is the FK program's store sink, c_sink)
    h.c_sink = o - kXf;
    o = (o + 3) & ~3;
    h.kpow2 = 1;
    while (h.kpow2 < K) h.kpow2 <<= 1;
    // Joint pass: (A) the distinct range sums read the site wrenches and go where the body transforms were (dead once the
    // site pass is over; the root position the moments refer to is read before); (B) the joints read those sums and write
    // the gradient where the site wrenches were.  Own region for the sums if they do not fit.
    h.c_gg = h.c_sw;
    if ((nst + 1) * kXf >= h.nrange * kXf) {
        h.c_rw = h.c_bx;
    } else {
        h.c_rw = o; o += h.nrange * kXf;
    }
    h.c_qe = h.c_sw;  // the evaluation point is dead once the site pass writes the wrenches (the LM kernel, which reads it
                      // later in the trip, moves it into its own region)
    // strides of 4 x odd words: regions stay 16-byte aligned (ds_read_b128 / ds_write_b128) and the chains of one
    // wavefront start in different banks
    auto stride_of = [](int words) { const int q = (words + 3) / 4; return kXf == 8 ? 4 * (q | 1) : (words | 1); };
    o = (o + 3) & ~3;
    h.stride_regs = stride_of(o) + std::max(m->dbg.stride_add, 0);
    h.stride_forced = m->dbg.stride_add >= 0;
    h.c_r2 = o; o += K > 64 ? h.kpow2 : ((K + 3) & ~3);
    h.c_kp = o; o += 3 * K;
    h.stride_lds = stride_of(o) + std::max(m->dbg.stride_add, 0);

    m->h_brec = brec; m->h_lev_adr = lev_adr; m->h_ab_jadr = ab_jadr; m->h_ab_jnum = ab_jnum; m->h_xf = xf;
    m->h_aj_pos = aj_pos;
    m->h_bpos.resize((size_t)3 * nab);
    for (int s = 0; s < nab; ++s)
        for (int i = 0; i < 3; ++i) m->h_bpos[3 * s + i] = brec[s].pos[i];
    bool any_bquat = false;
    for (int s = 0; s < nab; ++s) any_bquat = any_bquat || !(brec[s].flags & 1);
    {   // Split kinematics (PlanHeader::fk3; stac_plan.hpp): a free root at qpos 0 .. 6 on the ONE top-level active body, hinges
        // below it, no oriented body.  The lean kernels run nothing else, so a model without it takes the generic kernels.
        h.fk3 = 0;
        // (the free root's own body may be oriented: a free joint sets the body's pose, body_pos / body_quat do not enter -- mouse;
        //  an oriented body below it is one more product of P1, q_parent * body_quat, with the constant as its right factor -- fly)
        std::vector<float> bq_const;
        for (int s2 = 1; s2 < nab; ++s2)
            if (!(brec[s2].flags & 1)) bq_const.insert(bq_const.end(), brec[s2].quat, brec[s2].quat + 4);
        const int nbq = (int)bq_const.size() / 4;
        bool ok = naj >= 1 && aj_type[0] == STAC_JNT_FREE && aj_qadr[0] == 0 && ab_jnum[0] >= 1 && ab_jadr[0] == 0 && nqj == 1 && !has_ball &&
                  !m->dbg.nofk3 && !(nbq > 0 && m->dbg.nofk3bq);
        for (int j = 1; j < naj && ok; ++j) ok = aj_type[j] == STAC_JNT_HINGE;
        for (int s = 1; s < nab && ok; ++s) ok = ab_parent[s] != 0;
        if (ok) {
            PlanHeader g = h;  // the lean chain layout: regions of whole 4-word groups, stride 4 x odd (16-byte aligned entries)
            // capacities of a program area: the full program's own sizes (a pruned program is a sub-DAG: it is checked against them)
            Fk3Program probe;
            g.c3_qb = 0; g.c3_pb = 0; g.c3_ql = 0; g.c3_bq = 0; g.nbq = nbq; g.stride3 = 1;
            ok = build_fk3_program(m, g, nullptr, 254, 4096, 252, probe);
            if (ok) {
                // (cap1 even, >= 10: the table area 16 (cap1 + 2) holds cap1 / 2 + 3 records of 24 words; cap2: whole rounds of 32 lanes; cap3: whole blocks)
                g.fk3_cap1 = std::max(probe.n1, 10); g.fk3_cap2 = std::max((probe.n2 + 31) & ~31, 32); g.fk3_cap3 = std::max(probe.n3, 4);
                int o3 = 0;
                g.c3_qb = o3; o3 += (naj + 1 + nbq) * 4;                 // (+ 1: the sink of idle P1 positions; then the oriented bodies' nodes)
                g.c3_pb = o3; o3 += ((g.fk3_cap3 * 4 + 4) * 3 + 3) & ~3;  // (step, position) slots, root position, sink, slack of the prefetch
                g.c3_ql = o3; o3 += std::max(naj * 4, (h.nrange * kXf + 3) & ~3);
                g.c_rw = g.c3_ql;                                         // a full trip's range sums go where the joint-local quaternions were
                g.c3_rw0 = o3; o3 += 8;
                g.c3_bq = o3; o3 += 4 * nbq;                              // body_quat (w, x, y, z) of the oriented bodies: constants, written by the prologue
                g.c_jn = o3; o3 += 4;
                g.c_qsv = o3; o3 += 4 * nqj;
                g.c_sw = o3; o3 += (std::max(K * kXf, h.nqpad + kXf) + 3) & ~3;
                g.c_sink = g.c_sw + std::max(K * kXf, h.nqpad + kXf) - kXf;
                g.c_gg = g.c_qe = g.c_sw;
                g.c_bx = g.c_ja = 0;  // (unused by the lean kernels)
                const int q4 = (o3 + 3) / 4;
                g.stride3 = 4 * (q4 | 1);
                if ((g.stride3 / 4) % 8 == 0) g.stride3 += 8;  // (never a multiple of 32 words: the chains of a wavefront on different banks)
                g.stride_regs = g.stride_lds = g.stride3;
                g.stride_forced = 1;  // (q_chain_stride takes it as it is)
                Fk3Program full;
                ok = build_fk3_program(m, g, nullptr, g.fk3_cap1, g.fk3_cap2, g.fk3_cap3, full);
                if (ok) {
                    g.fk3 = 1;
                    g.fk3_n = full.n1 | full.n3 << 8 | full.n2 << 16;
                    g.off3_bq = put_raw(bq_const.data(), bq_const.size());
                    g.off3_prog = put_raw(full.words.data(), full.words.size());
                    g.off3_site = g.off3_prog + 16 * (g.fk3_cap1 + 2) + 4 * g.fk3_cap2 + 4 * g.fk3_cap3;
                    std::vector<int32_t> blank3(full.words.size(), 0);
                    g.off3_root = put_raw(blank3.data(), blank3.size());
                    // what both layouts share
                    const int32_t keep[] = {g.fk3, g.off3_site, g.off3_prog, g.off3_root, g.fk3_n,
                                            g.fk3_cap1, g.fk3_cap2, g.fk3_cap3};
                    h.fk3 = keep[0]; h.off3_site = keep[1]; h.off3_prog = keep[2]; h.off3_root = keep[3]; h.fk3_n = keep[4];
                    h.fk3_cap1 = keep[5]; h.fk3_cap2 = keep[6]; h.fk3_cap3 = keep[7];
                    h.c3_ql = g.c3_ql; h.c3_qb = g.c3_qb; h.c3_pb = g.c3_pb; h.c3_rw0 = g.c3_rw0; h.stride3 = g.stride3;
                    h.c3_bq = g.c3_bq; h.off3_bq = g.off3_bq; h.nbq = g.nbq;
                    m->h3 = g;
                }
            }
        }
    }
    {   // FK program (FkStep records, see stac_plan.hpp); a second area of the same size takes the pruned program of
        // the root passes, which depends on the call's trunk keypoints (fill_root_program)
        h.fk_rec_words = any_bquat ? 16 : 12;
        {   // header of a program area: a flag word per micro-level (of the full program: a pruned one has fewer),
            // then the first step's ql offset per position
            int mm = 0;
            for (int l = 0; l < nlev; ++l) {
                int ml = 1;
                for (int s2 = lev_adr[l]; s2 < lev_adr[l + 1]; ++s2) ml = std::max(ml, ab_jnum[s2]);
                mm += ml;
            }
            h.n_mlev_hdr = std::max((mm + 1) & ~1, 2);
            h.fk_hdr_words = ((h.n_mlev_hdr >> 1) + h.max_width + 3) & ~3;  // one flag word per pair of micro-levels
        }
        int n_mlev = 0;
        const std::vector<int32_t> prog = build_fk_program(m, nullptr, &n_mlev, &h.fk_uniform);  // (a pruned program is a subset)
        h.off_fkstep = put_raw(prog.data(), prog.size());
        h.n_mlev = n_mlev;
        std::vector<int32_t> blank(prog.size(), 0);
        h.off_fkroot = put_raw(blank.data(), blank.size());
        m->n_mlev_root = 0;
    }
    h.total_words = (int)B.size();

    h.chain_stride = h.stride_lds;
    if (!h.fk3) { m->off_wsum = 0; m->wsum = WsumProgram{}; }  // (no lean kernel after all: nobody stages the table)
    if (h.fk3) {  // the lean layout's copy of everything that was settled after it was made
        PlanHeader &g = m->h3;
        g.fk_rec_words = h.fk_rec_words; g.n_mlev_hdr = h.n_mlev_hdr; g.fk_hdr_words = h.fk_hdr_words; g.off_fkstep = h.off_fkstep;
        g.off_fkroot = h.off_fkroot; g.n_mlev = h.n_mlev; g.fk_uniform = h.fk_uniform; g.total_words = h.total_words;
        g.chain_stride = g.stride3;
        if (m->off_wsum) {  // the sweeps' store words: the range sums' entries, and for a sum that is nobody's the root fast trip's entry
                            // (c3_rw0: a full trip does not touch it, and a root fast trip writes it before it reads it)
            if (g.c_rw + kXf * h.nrange > 0xFFFF || g.c3_rw0 + kXf > 0xFFFF) return fail(STAC_ERR_CAPACITY, "plan: chain region too large for the wrench-sum program");
            const std::vector<int32_t> tab = m->wsum.table(g.c_rw, g.c3_rw0);
            std::memcpy(B.data() + m->off_wsum, tab.data(), tab.size() * sizeof(int32_t));
        }
    }
    return STAC_OK;
}

// LDS diet (PlanHeader::plan_skip): the offsets of the staged areas as the kernel sees them, from the first staged word
void rebase_plan_offsets(PlanHeader &h) {
    const int sk = h.plan_skip;
    if (sk <= 0) return;
    int32_t *offs[] = {&h.off_joint, &h.off_site, &h.off_range, &h.off_lb, &h.off_ub, &h.off_qpos0, &h.off_quat_adr,
                       &h.off_active, &h.off_fkstep, &h.off_fkroot, &h.off3_site, &h.off3_prog, &h.off3_root, &h.off3_bq};
    for (int32_t *o : offs) *o -= sk;
    h.off_lev_adr = h.off_body = 0;  // not staged (nothing of a program launch reads them)
}

int q_mb_words(int nkinds, int G) { return ((nkinds + 1) * G + 3) & ~3; }  // per-kind mask bits + one row of active-coordinate bits
// (G = 16: two chains share a 32-lane half of the wavefront, and the 32-bit LDS accesses bank by word address mod 32 per
// half: a stride of 16 mod 32 puts the second chain's run of 16 consecutive words on the other 16 banks.  Measured on the
// bench, profiles/r03/stride_sweep.txt: conflict cycles 25 % -> 16 % of the LDS-active ones; time within the noise,
// as it is for a stride of 0 mod 32 with 46 % -- the conflicts are not what the kernel waits for.)
int q_chain_stride(const PlanHeader &h, int G) {
    int s = h.K <= kSiteRounds * G ? h.stride_regs : h.stride_lds;
    if (G == 16 && kXf == 7 && !h.stride_forced) s += (16 - s % 32 + 32) % 32;
    return s;
}
size_t q_lds_bytes(const PlanHeader &h, int G, int nkinds, int wpb) {
    const int plan_words = (h.total_words - h.plan_skip + 3) & ~3;  // h is the per-launch copy: [plan_skip, total_words) = what this launch stages
    return (size_t)(plan_words + q_mb_words(nkinds, G) + wpb * (64 / G) * q_chain_stride(h, G)) * sizeof(float);
}

// Workgroups of wpb wavefronts that a CU holds (lds_bytes <= kLdsPerCu): LDS is allocated in granules (1280 B observed on gfx950:
// five 32 224-B workgroups do not fit a CU), and a register cap of waves_per_simd wavefronts per SIMD holds up to four waves of a
// workgroup spread over the SIMDs (only the CU total matters); a bigger workgroup puts ceil(wpb / 4) waves on some SIMD (the
// worst stacking is assumed).
int blocks_per_cu(size_t lds_bytes, int wpb, int waves_per_simd) {
    constexpr size_t kGranule = 1280;
    const int blocks = (int)(kLdsPerCu / ((lds_bytes + kGranule - 1) / kGranule * kGranule));
    return std::min(blocks, wpb <= 4 ? 4 * waves_per_simd / wpb : waves_per_simd / ((wpb + 3) / 4));
}

// Launch shape for a given G: wavefronts per workgroup (the waves of a block share one plan copy, so more chains fit the 160 KiB
// of a CU) and the register-cap variant of `kind` (kThr or kThrLean).  wpe = 2 keeps everything in registers (<= 256 VGPRs,
// 8 waves per CU); wpe = 3 (<= 168 VGPRs, 16-lane groups only) holds up to twelve waves as ONE workgroup (eleven: 3,3,3,2 over
// the SIMDs; two 5-wave workgroups could stack four waves on a SIMD -- the lean rodent layout fits eleven: 100 000 frames 649 ->
// 720 k frames/s); wpe = 4 (<= 128 VGPRs, more spills to scratch) admits 16 waves per CU.
QShape pick_shape(const PlanHeader &h, int G, int nkinds, int cus, long waves_needed, QKind kind) {
    QShape best{0, 2, 0};
    for (int wpe = 2; wpe <= 4; ++wpe) {
        if (!q_shape(kind, G, h.nq, wpe).nqr) continue;  // (only shapes that pass the spill gate are built: stac_shapes.hpp)
        for (int wpb = 1; wpb <= (wpe == 3 ? 12 : 8); ++wpb) {
            const size_t lds = q_lds_bytes(h, G, nkinds, wpb);
            if (lds > kLdsPerCu) break;
            const int waves = blocks_per_cu(lds, wpb, wpe) * wpb;
            // prefer more resident waves, then the smaller workgroup; a variant with a tighter register cap (more
            // spills) has to bring at least 20 % more waves than the best roomier one
            if (wpe == best.wpe ? waves > best.waves_per_cu : waves * 5 >= best.waves_per_cu * 6) best = QShape{wpb, wpe, waves};
            // few chains: the first shape that holds every wave at once is enough -- small workgroups spread
            // over more CUs and the 2-waves-per-SIMD variant does not spill
            if (waves_needed >= 0 && (long)waves * cus >= waves_needed) return QShape{wpb, wpe, waves};
        }
    }
    return best;
}

// ---- latency (speculative) mode: eight evaluation roles of G lanes per chain -------------------------------------------
// G = 8: one chain per wavefront, `chains` wavefronts per workgroup; G = 32 / 64: one chain per workgroup of 4 / 8
// wavefronts.  A chain's LDS block = 8 role regions + the exchange area (accept flags, losses, two gradients).
static int spec_xch_words(const PlanHeader &h) { return 64 + 4 * h.nqpad + 4; }
// nr = evaluation roles per chain: 8, or 4 (two chains per wavefront at 8 lanes per role: large batches)
size_t spec_lds_bytes(const PlanHeader &h, int G, int nkinds, int chains, int nr) {
    const int plan_words = (h.total_words - h.plan_skip + 3) & ~3;
    // (+ 1 KB: the range sums of the latency kernels read up to 23 site entries behind a range's end -- unclamped addresses, the values
    //  dropped --, which behind the workgroup's last chain would leave the allocation)
    return (size_t)(plan_words + q_mb_words(nkinds, G) + chains * (nr * q_chain_stride(h, G) + spec_xch_words(h))) * sizeof(float) + 1024;
}
// The one-wavefront-per-chain latency kernel (kLatG lanes per role: straggler hand-off, large clip counts) exists up to 8
// solver registers per lane (stac_shapes.hpp); wider models run four wavefronts per chain and keep their stragglers
bool lat_one_wave_ok(const PlanHeader &h) { return h.nq <= 16 * 8; }
SpecShape pick_spec_shape(const PlanHeader &h, int G, int nkinds, int cus, long nchains, int nr) {
    SpecShape best{G, 0, 0, 0};
    if ((G == 8 || G == 16) && G * nr <= 64) {  // 256-VGPR kernel: two waves per SIMD, eight per CU; 64 / (G nr) chains per wavefront
        const int cw = 64 / (G * nr);
        for (int w = 1; w <= 8; ++w) {
            const size_t lds = spec_lds_bytes(h, G, nkinds, w * cw, nr);
            if (lds > kLdsPerCu) break;
            const long res = (long)blocks_per_cu(lds, w, 2) * w * cw * cus;
            if (res > best.resident) best = SpecShape{G, w * cw, w, res};
            if (nchains >= 0 && res >= nchains) return SpecShape{G, w * cw, w, res};  // small workgroups spread over more CUs
        }
        return best;
    }
    const int nw = G * nr / 64;  // wavefronts per chain; 256-VGPR kernels as well (the 128-VGPR builds spill > 100 registers): eight waves per CU
    const size_t lds = spec_lds_bytes(h, G, nkinds, 1);
    if (lds > kLdsPerCu) return best;
    return SpecShape{G, 1, nw, (long)blocks_per_cu(lds, nw, 2) * cus};
}

// A lean instantiation of `kind` at G lanes (kThrLean: register cap `third`; kLatLean: `third` roles) that holds the model's nq
// coordinates and its K sites in registers -- the lean kernels have no LDS path for them: K <= lean_site_rounds(G, NQR) * G
bool lean_holds(const PlanHeader &h, QKind kind, int G, int third) {
    const int nqr = q_shape(kind, G, h.nq, third).nqr;
    return nqr > 0 && h.K <= lean_site_rounds(G, nqr) * G;
}
bool thr_lean_holds(const PlanHeader &h, int G) { return lean_holds(h, kThrLean, G, 2) || lean_holds(h, kThrLean, G, 3); }

// The active bodies a root pass needs: the ancestors of the weighted (trunk) keypoints' bodies.  Returns their number.
int root_pass_bodies(const stac_model *m, const uint8_t *trunk_kps, std::vector<char> &need) {
    need.assign(m->h.nab, 0);
    int n_need = 0;
    for (int k = 0; k < m->h.K; ++k)
        if (trunk_kps[k])
            for (int sl = m->h_site_slot[k]; sl >= 0 && !need[sl]; sl = m->h_ab_parent[sl] - 1) { need[sl] = 1; ++n_need; }
    return n_need;
}

// Diagnostics, not part of include/stac_hip.h (tests/test_fk3_rounds_host.py, tests/test_gpu_fk3_rounds.py): the split-kinematics
// program of a model, built on the host alone -- no device is touched.  trunk_kps == NULL: the full program; else the pruned program
// of the root passes for these trunk keypoints.  info[12] = {1 if the model takes the split kinematics, n1, n2, n3, rotations before
// the padding, cap2, the no-op task's quaternion word, the sink word of P2, distinct site ranges, PlanHeader::rsplit, active bodies,
// bodies the program evaluates}; t2 (may be NULL): the first min(cap2, cap_tasks) tasks of
// the program's T2 area, four words each.  Returns STAC_OK, or an error if the plan cannot be built.
extern "C" int32_t stac_debug_fk3_program(const stac_model_tables *t, const uint8_t *trunk_kps, int32_t *info, int32_t *t2, int32_t cap_tasks) {
    if (!t || !info) return fail(STAC_ERR_INVALID, "null argument");
    stac_model m;
    m.dbg.read_env();
    if (const int rc = build_plan(&m, t)) return rc;
    for (int i = 0; i < 12; ++i) info[i] = 0;
    info[8] = m.h.nrange; info[9] = m.h.rsplit; info[10] = m.h.nab;
    if (!m.h.fk3) return STAC_OK;
    const PlanHeader &h = m.h;
    Fk3Program pr;
    std::vector<char> need;
    info[11] = trunk_kps ? root_pass_bodies(&m, trunk_kps, need) : h.nab;
    if (!build_fk3_program(&m, m.h3, trunk_kps ? need.data() : nullptr, h.fk3_cap1, h.fk3_cap2, h.fk3_cap3, pr))
        return fail(STAC_ERR_CAPACITY, "the split-kinematics program does not fit the model's program area");
    info[0] = 1; info[1] = pr.n1; info[2] = pr.n2; info[3] = pr.n3; info[4] = pr.nrot; info[5] = h.fk3_cap2;
    info[6] = m.h3.c3_qb; info[7] = m.h3.c3_pb + 3 * (h.fk3_cap3 * 4 + 1);
    if (t2) std::memcpy(t2, pr.words.data() + 16 * (h.fk3_cap1 + 2), sizeof(int32_t) * 4 * (size_t)std::max(0, std::min(h.fk3_cap2, cap_tasks)));
    return STAC_OK;
}

// Diagnostics, as stac_debug_fk3_program (tests/test_wrench_sweep_host.py, tests/test_gpu_wrench_sweeps.py): the wrench-sum program of a
// model (WsumRec, stac_plan.hpp), built on the host alone.  out[0 .. 23] = {1 if the model has a program, component tasks, whole ranges,
// rows, depth, row_start[0 .. 2], distinct ranges, K, words of the table, words a lean throughput launch without root program stages,
// its chain stride at 16 lanes, its LDS bytes for one wavefront per workgroup and three solve kinds (q_lds_bytes), the words of its
// mask table, kXf, c_sw, c_rw of the lean layout, PlanHeader::rsplit, the staged words without the table, c3_rw0 (the sweeps' dump
// entry), c3_ql, stride3, 0}; then {lo, hi} of every
// distinct range; then the table.  Nothing beyond out[cap_words) is written; returns STAC_OK, or an error if cap_words is too small.
extern "C" int32_t stac_debug_wsum_program(const stac_model_tables *t, int32_t *out, int32_t cap_words) {
    if (!t || !out) return fail(STAC_ERR_INVALID, "null argument");
    stac_model m;
    m.dbg.read_env();
    if (const int rc = build_plan(&m, t)) return rc;
    const std::vector<float> &B = m.blob_host;
    const std::vector<int32_t> tab = m.wsum.table(0, 0);
    const int need = 24 + 2 * m.h.nrange + (int)tab.size();
    if (cap_words < need) return fail(STAC_ERR_CAPACITY, "stac_debug_wsum_program: the buffer is too small");
    for (int i = 0; i < need; ++i) out[i] = 0;
    out[8] = m.h.nrange; out[9] = m.h.K; out[15] = kXf; out[18] = m.h.rsplit;
    std::memcpy(out + 24, B.data() + m.h.off_range, sizeof(int32_t) * 2 * (size_t)m.h.nrange);
    if (!m.off_wsum) return STAC_OK;
    out[0] = 1; out[1] = m.wsum.ntask; out[2] = m.wsum.nwhole; out[3] = m.wsum.nrows; out[4] = m.wsum.depth;
    for (int i = 0; i < 3; ++i) out[5 + i] = m.wsum.row_start[i];
    out[10] = (int)tab.size();
    PlanHeader hh = m.h3;  // (plan_q, lean_header(true), without the root program)
    hh.plan_skip = m.off_wsum;
    hh.total_words = hh.off3_root;
    out[11] = hh.total_words - hh.plan_skip; out[12] = q_chain_stride(hh, 16); out[13] = (int32_t)q_lds_bytes(hh, 16, 3, 1);
    out[14] = q_mb_words(3, 16); out[16] = hh.c_sw; out[17] = hh.c_rw; out[19] = hh.off3_root - (m.h.off_joint - 2 * kTTab);
    out[20] = hh.c3_rw0; out[21] = hh.c3_ql; out[22] = hh.stride3;
    std::memcpy(out + 24 + 2 * m.h.nrange, B.data() + m.off_wsum, sizeof(int32_t) * tab.size());  // (what the launch stages, not a copy of it)
    return STAC_OK;
}
