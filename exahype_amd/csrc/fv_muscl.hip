// MUSCL-Hancock patch update (exa_fv_muscl.hpp) for the built-in term sets: Euler and the advection, 2-D and 3-D.  EulerRef2D is the reference's
// quirk set (F[4] is never written): exa_fv_plan_create refuses it in this mode, its slot stays null.
#include "exa_fv_muscl.hpp"

namespace exa {

void fv_muscl_fill_builtin(PdeKernels* tab) {
    tab[1].fv_muscl = fv_muscl_entry<Euler>;
    tab[2].fv_muscl = fv_muscl_entry<Advection<FVM_MAXV>>;
}

}  // namespace exa
