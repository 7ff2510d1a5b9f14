/* Host build of include/md_contact_response.h, loaded by the tests through tests/hostlib.py: one md_contact_response launch
 * restated as a plain loop over the envs (all pointers host arrays), the pieces of the rule for the geometry and known-answer
 * tests, md_obb_obb / md_obb_circle of md_geom.h on the same records, and sizeof(MdContactResponse) as the C compiler sees it. */
#include "md_contact_response.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_contact_response(void) { return (int)sizeof(MdContactResponse); }

/* md_contact_response without the launch */
EXPORT int hx_contact_response(const MdState* s, const MdConfig* c, const MdContactResponse* cr) {
    for (int e = 0; e < c->n_envs; ++e) {
        const MdState v = md_env_view(s, c, e);
        md_contact_response_env(&v, c, cr, e);
    }
    return 0;
}

/* n pairs: responder record I[k] in slot si[k] against obstacle record J[k] in slot sj[k] -> out[4 k ..] = hit, depth, nx, ny;
 * near[k] = md_cr_near; ref[k] = md_obb_obb / md_obb_circle on the same floats */
EXPORT void hx_cr_contacts(const MdShape* I, const int* si, const MdShape* J, const int* sj, int n, float* out, int* near, int* ref) {
    for (int k = 0; k < n; ++k) {
        const MdCrHit h = md_cr_contact(&I[k], si[k], &J[k], sj[k]);
        out[4 * k] = (float)h.hit;
        out[4 * k + 1] = h.depth;
        out[4 * k + 2] = h.nx;
        out[4 * k + 3] = h.ny;
        near[k] = md_cr_near(&I[k], &J[k]);
        if (md_is_circle_kind(md_kind_of(J[k].flags)))
            ref[k] = md_obb_circle(I[k].cx, I[k].cy, I[k].c, I[k].s, I[k].hl, I[k].hw, J[k].cx, J[k].cy, J[k].hl);
        else {
            const MdShape* A = si[k] < sj[k] ? &I[k] : &J[k];    /* (lo, hi), as the rule evaluates the pair */
            const MdShape* B = si[k] < sj[k] ? &J[k] : &I[k];
            ref[k] = md_obb_obb(A->cx, A->cy, A->c, A->s, A->hl, A->hw, B->cx, B->cy, B->c, B->s, B->hl, B->hw);
        }
    }
}
