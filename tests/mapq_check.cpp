// mapq_check.cpp -- csrc/map_quality_device.h compiled for the host (tests/test_mapq_host.py): the cell index and the whole
// per-query chain (membership, moments, covariance, eigen-pair, entropy) exactly as the kernels of map_quality.hip run it, with
// the candidates visited in index order.
#include <cstdint>
#include "../global-lvba_amd/csrc/map_quality_device.h"

using namespace lvba;

extern "C" {

double emul_cell_edge(double radius) { return mapq_cell_edge(radius); }

// cells [n][3]; ok[i] = 0: non-finite, 1: in range, 2: finite but out of range
void emul_cells(int64_t n, const float *xyz, double radius, int64_t *cells, uint8_t *ok)
{
    const double edge = mapq_cell_edge(radius);
    for (int64_t i = 0; i < n; ++i) {
        int64_t c[3] = {0, 0, 0};
        ok[i] = 0;
        if (mapq_finite(xyz + 3 * i)) ok[i] = mapq_cell_of(xyz + 3 * i, edge, c) ? 1 : 2;
        for (int j = 0; j < 3; ++j) cells[3 * i + j] = c[j];
    }
}

uint64_t emul_pack(int64_t x, int64_t y, int64_t z) { return mapq_pack(x, y, z); }

void emul_metrics(int64_t n, const float *xyz, double radius, int min_neighbors, int64_t stride, int32_t *count, uint8_t *valid,
                  double *entropy, double *plane_var, float *normal)
{
    const double r2 = radius * radius;
    for (int64_t i = 0, k = 0; i < n; i += stride, ++k) {
        MapqAcc a;
        mapq_clear(a);
        if (mapq_finite(xyz + 3 * i)) {
            const double wq[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
            for (int64_t j = 0; j < n; ++j)
                if (mapq_finite(xyz + 3 * j)) mapq_visit(a, wq, (double)xyz[3 * j], (double)xyz[3 * j + 1], (double)xyz[3 * j + 2], r2);
        }
        MapqOut o;
        mapq_finish(a, min_neighbors, o);
        count[k] = a.n;
        valid[k] = (uint8_t)o.valid;
        entropy[k] = o.entropy;
        plane_var[k] = o.plane_var;
        for (int j = 0; j < 3; ++j) normal[3 * k + j] = o.normal[j];
    }
}

}
