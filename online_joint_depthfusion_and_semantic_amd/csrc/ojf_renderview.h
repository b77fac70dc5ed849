// The view of the ray casts, shared by ojf_render.hip and ojf_color.hip: one struct and one host text that fills it, so
// that ojf_color_render's colours land on exactly the hit points ojf_render's depth image marks.
#pragma once
#include "ojf_common.h"

namespace ojf {

struct RenderView {  // by value in the kernel arguments
    float Ki[9];
    float R[9];  // E[:, :3], row-major
    float o[3];  // fp32((E[:,3] - origin) / res)
};

static inline void make_render_view(const float *Kinv, const float *E, const double *origin, double res, RenderView &V)
{
    for (int i = 0; i < 9; ++i) V.Ki[i] = Kinv[i];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) V.R[3 * i + k] = E[4 * i + k];
        V.o[i] = (float)(((double)E[4 * i + 3] - origin[i]) / res);
    }
}

}  // namespace ojf
