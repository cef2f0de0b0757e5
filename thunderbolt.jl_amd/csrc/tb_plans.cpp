// tb_plans.cpp — the device half of the assembly plans: the environment becomes plan::Options, the planners of tb_planners.cpp build the
// host arrays, and this file caches them on the mesh / pattern and uploads them (once per mesh / pattern, in front of any graph capture).
#include <cstring>

#include "tb_internal.h"

namespace tb {
using namespace plan;

static MeshView view(const tb_mesh *m) { return {m->n_nodes, m->n_cells, m->ndofs, m->nverts, m->ndpc, m->ncomp, m->h_xyz.data(), m->h_conn.data(), m->h_cell_dofs.data()}; }
static PatternView view(const tb_pattern *p) { return {p->n_rows, p->h_rowptr.data(), p->h_colidx.data(), p->max_row_len}; }

void ensure_max_row_len(tb_pattern *p)
{
    if (p->max_row_len) return;
    for (int64_t r = 0; r < p->n_rows; ++r) p->max_row_len = std::max<int64_t>(p->max_row_len, p->h_rowptr[r + 1] - p->h_rowptr[r]);
}

static bool parse3(const char *e, int *t)
{
    int a, b, c;
    if (!e || sscanf(e, "%d,%d,%d", &a, &b, &c) != 3 || a <= 0 || b <= 0 || c <= 0) return false;
    t[0] = a; t[1] = b; t[2] = c;
    return true;
}

// TB_PATCH_TILE="tx,ty,tz" overrides the tile; TB_PATCH_CELLS=n selects Morton runs of n cells instead; TB_VPATCH_TILE the vector plan's tile
static Options env_options()
{
    Options o;
    const char *tile = getenv("TB_PATCH_TILE"), *cells = tune_env("TB_PATCH_CELLS");
    o.tile_set = tile != nullptr;
    o.morton = !parse3(tile, o.tile) && cells;
    if (cells && atoi(cells) > 0) o.cells = atoi(cells);
    o.fixed = cells || tile;
    static const bool full_cut = getenv("TB_PATCH_CUT") && !strcmp(getenv("TB_PATCH_CUT"), "full"); // full tiles + sliver, for A/B runs; read once per process
    o.full_cut = full_cut;
    if (const char *e = tune_env("TB_PATCH_THREADS")) o.threads = atoi(e);
    parse3(tune_env("TB_VPATCH_TILE"), o.vtile);
    if (const char *e = tune_env("TB_PATCH_RCB")) o.vec_rcb = strcmp(e, "0") != 0;
    if (const char *e = tune_env("TB_RCB_MAX_INST")) o.rcb_max_inst = atoi(e);
    o.verbose = getenv("TB_PLAN_VERBOSE") != nullptr;
    return o;
}

int build_ea_plan(tb_mesh *m)
{
    if (m->n_cells * m->ndpc >= (int64_t)0x7fffffff) { set_error("element-assembly plan: too many slots for int32"); return TB_ERR_UNSUPPORTED; }
    std::vector<int64_t> ptr;
    std::vector<int32_t> src;
    dof_slots(view(m), ptr, src);
    auto plan = std::make_unique<EAPlan>();
    TB_TRY(upload_all(m->dev, ptr, &plan->d_ptr, src, &plan->d_src));
    TB_HIP(hipMalloc((void **)&plan->d_ea, sizeof(double) * m->n_cells * m->ndpc));
    m->ea = std::move(plan);
    return TB_OK;
}

int ensure_ea_ell(tb_mesh *m)
{
    if (!m->ea) { int rc = build_ea_plan(m); if (rc) return rc; }
    if (m->ea->d_ell) return TB_OK;
    SlotTable t = slot_table(view(m));
    TB_TRY(upload(m->dev, t.ell, &m->ea->d_ell));
    m->ea->ell_w = t.w;
    m->ea->h_done = std::move(t.h_done);
    return TB_OK;
}

int ensure_ea_ell_q2t(tb_mesh *m)
{
    TB_TRY(ensure_ea_ell(m));
    if (m->ea->d_ell_t) return TB_OK;
    TB_NO_CAPTURE(m->dev);
    if (m->ndpc != 27) { set_error("tensor-order slot table: needs 27 dofs per cell"); return TB_ERR_UNSUPPORTED; }
    std::vector<int32_t> ell((size_t)m->ndofs * m->ea->ell_w);
    TB_HIP(hipMemcpy(ell.data(), m->ea->d_ell, ell.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    tensor_order(ell);
    return upload(m->dev, ell, &m->ea->d_ell_t);
}

static int color_plan(tb_mesh *m, const int32_t *cells, int64_t n, std::unique_ptr<ColorPlan> &out)
{
    ColorHost h;
    TB_TRY(color_cells(view(m), cells, n, h));
    auto plan = std::make_unique<ColorPlan>();
    plan->ncolors = h.ncolors;
    plan->offsets = std::move(h.offsets);
    TB_TRY(upload(m->dev, h.cells, &plan->d_cells));
    out = std::move(plan);
    return TB_OK;
}

int build_color_plan(tb_mesh *m) { return color_plan(m, nullptr, m->n_cells, m->colors); }
int build_color_plan_subset(tb_mesh *m, const std::vector<int32_t> &cells, std::unique_ptr<ColorPlan> &out) { return color_plan(m, cells.data(), (int64_t)cells.size(), out); }

static void free_device(PatchPlan *pl)
{
    hipFree(pl->d_elem_ptr); hipFree(pl->d_row_ptr); hipFree(pl->d_elem_cell); hipFree(pl->d_elem_lrow); hipFree(pl->d_row_dof);
    pl->d_elem_ptr = pl->d_row_ptr = nullptr; pl->d_elem_cell = pl->d_row_dof = nullptr; pl->d_elem_lrow = nullptr;
}

void free_patch_plan(tb_mesh *m)
{
    if (!m->patches) return;
    free_device(m->patches.get());
    m->patches.reset();
}

void free_patch_mat_plan(tb_pattern *p)
{
    if (!p->patch_mat) return;
    hipFree(p->patch_mat->d_row_desc); hipFree(p->patch_mat->d_elem_rowoff); hipFree(p->patch_mat->d_colpos8); hipFree(p->patch_mat->d_colpos16);
    p->patch_mat.reset();
}

void free_patch_fused_plan(tb_pattern *p)
{
    if (!p->patch_fused) return;
    PatchFusedPlan *f = p->patch_fused.get();
    hipFree(f->d_node_ptr); hipFree(f->d_pnode); hipFree(f->d_elem_ln); hipFree(f->d_elem_sig); hipFree(f->d_sigtab); hipFree(f->d_row_desc); hipFree(f->d_hdr); hipFree(f->d_pcoord);
    hipFree(f->d_rec);
    p->patch_fused.reset();
}

void free_vec_patch_plans(tb_mesh *m)
{
    for (auto &v : m->vpatches) {
        if (!v) continue;
        hipFree(v->d_hdr); hipFree(v->d_elem_ln); hipFree(v->d_elem_cell); hipFree(v->d_pcoord); hipFree(v->d_pdof);
        v.reset();
    }
}

static_assert((int)plan::ERR_BAD_ARG == (int)TB_ERR_BAD_ARG && (int)plan::ERR_PATTERN == (int)TB_ERR_PATTERN && (int)plan::ERR_UNSUPPORTED == (int)TB_ERR_UNSUPPORTED, "the planners' codes are the ABI's");

// A fit edits the mesh's patch plan in place; where it replaced the host arrays (only the winning plan of a fit gets here) the device copies follow and
// the version moves on, which invalidates every extension built for the plan before.  A failed patch planner leaves no plan behind.
static int sync_patch_plan(tb_mesh *m, bool replaced, int version)
{
    if (!replaced) return TB_OK;
    PatchPlan *pl = m->patches.get();
    free_device(pl);
    if (pl->h_elem_ptr.empty()) { m->patches.reset(); return TB_OK; }
    PlanTimer timer("build_patch_plan"); // the planner printed its laps; "uploads" and "(rest)" close the builder's lines as before
    pl->version = version + 1;
    const int rc = upload_all(m->dev, pl->h_elem_ptr, &pl->d_elem_ptr, pl->h_row_ptr, &pl->d_row_ptr, pl->h_elem_cell, &pl->d_elem_cell, pl->h_elem_lrow, &pl->d_elem_lrow,
                              pl->h_row_dof, &pl->d_row_dof);
    if (rc) free_patch_plan(m);
    timer.lap("uploads");
    return rc;
}

// the mesh's patch plan as a fit expects it: the cached one, or an empty one to build into
static PatchPlan &patch_slot(tb_mesh *m, int &version)
{
    version = m->patches ? m->patches->version : 0;
    if (!m->patches) m->patches = std::make_unique<PatchPlan>();
    return *m->patches;
}

// Build the patch plan and (when a pattern is given) its matrix extension, fitted to the LDS budget (plan::fit_mat).  The planners run before any
// device call, so a refusal comes back as such while a graph capture is open too; upload() is what refuses inside a capture.
int ensure_patch_plans(tb_mesh *m, tb_pattern *p)
{
    if (m->patches && (!p || (p->patch_mat && p->patch_mat->version == m->patches->version))) return TB_OK;
    const Options o = env_options();
    bool replaced = !p;
    int version;
    PatchPlan &cur = patch_slot(m, version);
    Outcome r;
    MatHost h;
    if (p) r = fit_mat(view(m), view(p), o, m->fit, cur, replaced, h);
    else if (int rc = patch_plan(view(m), o, m->fit.patch_rcb, 0, cur)) { m->patches.reset(); return rc; }
    if (p) free_patch_mat_plan(p);
    TB_TRY(sync_patch_plan(m, replaced, version));
    if (!p) return TB_OK;
    if (!r.ok()) return r.code;
    p->patch_mat = std::make_unique<PatchMatPlan>();
    PatchMatPlan *d = p->patch_mat.get();
    d->version = m->patches->version;
    d->max_lds_entries = h.max_lds_entries;
    const int rc = upload_all(m->dev, h.row_desc, &d->d_row_desc, h.rowoff, &d->d_elem_rowoff, h.cp8, &d->d_colpos8, h.cp16, &d->d_colpos16);
    if (rc) free_patch_mat_plan(p);
    return rc;
}

// Build (or refit) the mesh's patch plan and the pattern's fused extension (plan::fit_fused).  The extension's host arrays are released on return.
int ensure_patch_fused(tb_mesh *m, tb_pattern *p, int nregions)
{
    if (const PatchFusedPlan *f = p->patch_fused.get())
        if (m->patches && f->version == m->patches->version && f->d_row_desc &&
            (int64_t)nregions * f->max_lds_entries * 8 + (int64_t)m->patches->max_rows * 16 + (int64_t)f->max_nodes * 24 <= LDS_BUDGET)
            return TB_OK;
    const Options o = env_options();
    bool replaced;
    int version;
    PatchPlan &cur = patch_slot(m, version);
    FusedHost h;
    if (m->nverts == 8 && m->ndpc == 8) ensure_max_row_len(p);
    const Outcome r = fit_fused(view(m), view(p), o, nregions, m->fit, cur, replaced, h);
    free_patch_fused_plan(p);
    TB_TRY(sync_patch_plan(m, replaced, version));
    if (!r.ok()) return r.code;
    p->patch_fused = std::make_unique<PatchFusedPlan>();
    PatchFusedPlan *d = p->patch_fused.get();
    d->version = m->patches->version;
    d->max_lds_entries = h.max_lds_entries; d->max_nodes = h.max_nodes; d->nsig = h.nsig;
    const int rc = upload_all(m->dev, h.node_ptr, &d->d_node_ptr, h.pnode, &d->d_pnode, h.ln, &d->d_elem_ln, h.elem_sig, &d->d_elem_sig, h.sigtab, &d->d_sigtab,
                              h.row_desc, &d->d_row_desc, h.hdr, &d->d_hdr, h.pcoord, &d->d_pcoord);
    if (rc) free_patch_fused_plan(p);
    return rc;
}

// One-trip records (PatchFusedPlan::d_rec), packed from the compact arrays read back from the device copies the plan already holds (the host vectors of
// the fused extension are gone by now; this runs once per pattern).
static int ensure_patch_records_impl(tb_pattern *p)
{
    PatchFusedPlan *f = p->patch_fused.get();
    const PatchPlan *pp = p->mesh->patches.get();
    if (!f || !pp || !f->d_hdr) return TB_ERR_UNSUPPORTED;
    if (f->d_rec) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    PlanTimer timer("ensure_patch_records_impl");
    Records rec = f->rec_stride < 0 ? Records() : record_layout(*pp, f->max_nodes);
    if (rec.stride < 0) { f->rec_stride = -1; return TB_ERR_UNSUPPORTED; }
    const int64_t np = pp->n_patches;
    std::vector<uint32_t> hdr((size_t)np * 4);
    std::vector<uint16_t> ln((size_t)pp->total_elems * 8);
    std::vector<uint32_t> sig((size_t)pp->total_elems);
    std::vector<RowDesc> desc((size_t)pp->total_rows);
    TB_HIP(hipMemcpy(hdr.data(), f->d_hdr, hdr.size() * 4, hipMemcpyDeviceToHost));
    TB_HIP(hipMemcpy(ln.data(), f->d_elem_ln, ln.size() * 2, hipMemcpyDeviceToHost));
    TB_HIP(hipMemcpy(sig.data(), f->d_elem_sig, sig.size() * 4, hipMemcpyDeviceToHost));
    TB_HIP(hipMemcpy(desc.data(), f->d_row_desc, desc.size() * sizeof(RowDesc), hipMemcpyDeviceToHost));
    int64_t total_nodes = 0;
    for (int64_t q = 0; q < np; ++q) total_nodes = std::max<int64_t>(total_nodes, (int64_t)hdr[4 * q + 2] + ((hdr[4 * q + 3] >> 10) & 0x7ff));
    std::vector<double> xyz((size_t)total_nodes * 3);
    TB_HIP(hipMemcpy(xyz.data(), f->d_pcoord, xyz.size() * 8, hipMemcpyDeviceToHost));
    std::vector<uint8_t> sigtab((size_t)f->nsig * 64);
    TB_HIP(hipMemcpy(sigtab.data(), f->d_sigtab, sigtab.size(), hipMemcpyDeviceToHost));
    const RecordClasses cls = classify_records(np, hdr.data(), ln.data(), sig.data(), desc.data(), sigtab.data());
    pack_records(rec, np, hdr.data(), ln.data(), sig.data(), desc.data(), xyz.data(), cls.order.data());
    TB_HIP(hipMalloc((void **)&f->d_rec, rec.bytes.size()));
    TB_HIP(hipMemcpy(f->d_rec, rec.bytes.data(), rec.bytes.size(), hipMemcpyHostToDevice));
    f->rec_stride = rec.stride; f->rec_rm = rec.rm; f->rec_nm = rec.nm; f->rec_ne = rec.ne;
    f->rec_general = cls.n_general; f->rec_canonical = cls.n_canonical;
    if (getenv("TB_PLAN_VERBOSE"))
        fprintf(stderr, "[tbhip] one-trip patch records: %lld patches x %zu B (rows <= %d, nodes <= %d), %.2f GB; %lld general, %lld canonical\n", (long long)np, (size_t)rec.stride, rec.rm, rec.nm,
                (double)rec.bytes.size() / 1e9, (long long)cls.n_general, (long long)cls.n_canonical);
    return TB_OK;
}

// A failure on the way (the records are ≈ 1 GB at 216³: the allocation can fail) is latched — rec_stride = −1, the sticky HIP error cleared — so that the
// following assemblies go straight to the staged kernel instead of repeating four device-to-host copies and a multi-GB host build per call.
int ensure_patch_records(tb_pattern *p)
{
    const int rc = ensure_patch_records_impl(p);
    if (rc != TB_OK && rc != TB_ERR_UNSUPPORTED) {
        PatchFusedPlan *f = p->patch_fused.get();
        if (f) {
            if (f->d_rec) { (void)hipFree(f->d_rec); f->d_rec = nullptr; }
            f->rec_stride = -1;
        }
        (void)hipGetLastError();
        return TB_ERR_UNSUPPORTED;
    }
    return rc;
}

int ensure_vec_patch_plan(tb_mesh *m, bool halo)
{
    if (m->vpatches[halo]) return TB_OK;
    VecHost h;
    TB_TRY(vec_patch_plan(view(m), env_options(), halo, h));
    auto &v = m->vpatches[halo];
    v = std::make_unique<VecPatchPlan>();
    v->halo = halo; v->n_patches = h.n_patches; v->total_elems = h.total_elems; v->total_nodes = h.total_nodes; v->max_nodes = h.max_nodes; v->max_elems = h.max_elems;
    const int rc = upload_all(m->dev, h.hdr, &v->d_hdr, h.ln, &v->d_elem_ln, h.ecell, &v->d_elem_cell, h.pcoord, &v->d_pcoord, h.pdof, &v->d_pdof);
    if (rc) { hipFree(v->d_hdr); hipFree(v->d_elem_ln); hipFree(v->d_elem_cell); hipFree(v->d_pcoord); hipFree(v->d_pdof); v.reset(); }
    return rc;
}

} // namespace tb
