// What hor3map.hip offers the library beside its C-ABI (include/blomgpu_hor3map.h): the calls of stage_ale.hip, which runs the grid on the
// model context's streams and inside blomgpu_step.  The comments at the definitions say what each does.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/blomgpu_hor3map.h"

int h3m_use_stream(blomgpu_h3m_grid *G, hipStream_t stream);
int h3m_set_stream(blomgpu_h3m_grid *G, hipStream_t stream);
int h3m_set_active(blomgpu_h3m_grid *G, const int *active);
int h3m_sequence_begin(blomgpu_h3m_grid *G);
int h3m_sequence_end(blomgpu_h3m_grid *G);
int h3m_sequence_begin_deferred(blomgpu_h3m_grid *G);
int h3m_sequence_end_deferred(blomgpu_h3m_grid *G);
int h3m_sequence_poll(blomgpu_h3m_grid *G, unsigned long long *column);
int h3m_extract_polycoeff_many(blomgpu_h3m_grid *G, int nf, blomgpu_h3m_src *const *srcs, double *const *outs);
