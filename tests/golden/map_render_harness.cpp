// tests/golden/map_render_harness.cpp -- TEST INFRASTRUCTURE ONLY (golden data for tests/golden/map_render.npz).
//
// A small program around the UNMODIFIED reference headers (slam_constructor's src/, given with -I): maps of every cell
// class the device path holds, filled through GridMap::update (and, for the hand-made edge cells, GridMap::reset), then
// read the way the reference's two map consumers read them -- (double)map[c] and the cell loop of
// OccupancyGridPublisher::on_map_update, and GridMapToPgmDumber::dump_map itself.
// tests/golden/make_golden_map_render.py compiles it (g++ -std=c++14 -O3, the reference's own flags), feeds it one file
// of doubles and packs what it writes; the binary is never committed and nothing in the product path knows about it.
//
//   map_render_harness <input.bin> <output.bin> <scratch.pgm>
//
// Input and output are flat arrays of doubles in the order read / written below.  Access control is relaxed only so
// that hand-made states can be put into a cell and the map's origin can be moved off its centre.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#define private public
#define protected public
#include "core/maps/plain_grid_map.h"
#include "core/maps/naive_grid_cells.h"
#include "core/maps/tbm_grid_cells.h"
#include "slams/gmapping/gmapping_grid_cell.h"
#include "slams/credibilist/grid_cell.h"
#include "utils/map_dumpers.h"
#undef private
#undef protected

namespace {

std::vector<double> in_buf, out_buf;
size_t in_pos = 0;
std::string pgm_path;
double rd() {
  if (in_pos >= in_buf.size()) {
    std::fprintf(stderr, "map_render_harness: input too short\n");
    std::exit(2);
  }
  return in_buf[in_pos++];
}
int rdi() { return (int)rd(); }
void wr(double v) { out_buf.push_back(v); }

// cell classes in the generator's order
enum { AFFINE = 0, MEAN = 1, TBM_CONSISTENT = 2, TBM_UNKNOWN_EVEN = 3, GMAPPING = 4, CREDIBILIST = 5 };

std::shared_ptr<GridCell> prototype(int cls) {
  switch (cls) {
    case AFFINE: return std::make_shared<AffineQualityMergeCell>();
    case MEAN: return std::make_shared<MeanProbabilityCell>();
    case TBM_CONSISTENT: return std::make_shared<TbmOccConsistentCell>();
    case TBM_UNKNOWN_EVEN: return std::make_shared<TbmUnknownEvenOccCell>();
    case GMAPPING: return std::make_shared<GmappingBaseCell>();
    default: return std::make_shared<CredibilistCell>();
  }
}

// the cell's payload in the device library's host stride
void write_payload(int cls, const GridCell &c) {
  if (cls == AFFINE || cls == MEAN) {
    wr(c.occupancy().prob_occ);
  } else if (cls == GMAPPING) {
    const auto &g = static_cast<const GmappingBaseCell &>(c);
    wr(g.occupancy().prob_occ);
    wr(g.obst.x);
    wr(g.obst.y);
  } else {
    const TBM &t = cls == CREDIBILIST ? static_cast<const CredibilistCell &>(c).belief()
                                      : static_cast<const TbmBaseCell &>(c).belief();
    wr(t.unknown());
    wr(t.empty());
    wr(t.occupied());
    wr(t.conflict());
  }
}

// geometry, payloads, (double)map[c], the publisher's int8 and the dumper's bytes; cells in internal order, y ascending
void emit(int cls, const GridMap &map) {
  const int w = map.width(), h = map.height();
  const DiscretePoint2D origin = map.origin();
  wr(w);
  wr(h);
  wr(origin.x);
  wr(origin.y);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) write_payload(cls, map[{x - origin.x, y - origin.y}]);
  // OccupancyGridPublisher::on_map_update's three lines per cell (src/ros/occupancy_grid_publisher.h:42-44) restated
  // -- the ROS headers it includes are not available -- over the cells in this harness's own order (y, then x,
  // ascending).  9999 = the conversion is undefined for this value (not finite, or its hundredfold outside int):
  // such a cell has no golden byte.
  std::vector<double> values, bytes;
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      const DiscretePoint2D pnt{x - origin.x, y - origin.y};
      double value = (double)map[pnt];
      values.push_back(value);
      if (!std::isfinite(value) || !(std::fabs(value * 100) < 2147483647.0)) {
        bytes.push_back(9999);
        continue;
      }
      int cell_value = value == -1 ? -1 : value * 100;
      std::vector<int8_t> data;
      data.push_back(cell_value);
      bytes.push_back(data.back());
    }
  }
  for (double v : values) wr(v);
  for (double v : bytes) wr(v);
  // GridMapToPgmDumber::dump_map, the reference's own code, into a scratch file; header checked, pixels kept
  {
    std::ofstream scratch(pgm_path, std::ios::out | std::ios::binary | std::ios::trunc);
    GridMapToPgmDumber::dump_map(scratch, map);
  }
  FILE *f = std::fopen(pgm_path.c_str(), "rb");
  if (!f) std::exit(3);
  std::vector<unsigned char> file(1 << 20);
  file.resize(std::fread(file.data(), 1, file.size(), f));
  std::fclose(f);
  const std::string header = "P5\n" + std::to_string(w) + "\n" + std::to_string(h) + "\n255\n";
  if (file.size() != header.size() + (size_t)w * h || std::string(file.begin(), file.begin() + header.size()) != header) {
    std::fprintf(stderr, "map_render_harness: unexpected PGM header or size\n");
    std::exit(4);
  }
  for (size_t i = header.size(); i < file.size(); ++i) wr(file[i]);
}

// a cell of class cls holding the hand-made state s[0..3]: the occupancy itself (s[0]) for the one-value classes and
// the GMapping cell, the belief (u, e, o, c) for the others -- whose occupancy is then derived by the class's own
// conversion; the vacuous belief stays the fresh cell (a TbmBaseCell keeps its prototype's occupancy until updated)
std::shared_ptr<GridCell> edge_cell(int cls, const double *s) {
  auto cell = prototype(cls);
  if (cls == AFFINE || cls == MEAN || cls == GMAPPING) {
    cell->_occupancy.prob_occ = s[0];
  } else if (s[0] == 1.0 && s[1] == 0.0 && s[2] == 0.0 && s[3] == 0.0) {
    // fresh
  } else if (cls == CREDIBILIST) {
    auto &c = static_cast<CredibilistCell &>(*cell);
    c._belief = TBM(s[0], s[1], s[2], s[3]);
    c.refresh_grid_cell();
  } else {
    auto &c = static_cast<TbmBaseCell &>(*cell);
    c._belief = TBM(s[0], s[1], s[2], s[3]);
    c._occupancy = c.tbm2occ(c._belief);
  }
  return cell;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) return 1;
  pgm_path = argv[3];
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in_buf.resize(bytes / sizeof(double));
    if (std::fread(in_buf.data(), sizeof(double), in_buf.size(), f) != in_buf.size()) return 1;
    std::fclose(f);
  }
  const int n_classes = rdi();
  for (int k = 0; k < n_classes; ++k) {
    const int cls = rdi();
    // ---- a map filled through GridMap::update ----
    const int w = rdi(), h = rdi();
    const double scale = rd();
    const int ox = rdi(), oy = rdi();
    UnboundedPlainGridMap map(prototype(cls), GridMapParams{w, h, scale});
    map._origin = DiscretePoint2D{ox, oy};
    const int n_obs = rdi();
    for (int i = 0; i < n_obs; ++i) {
      const int x = rdi(), y = rdi();
      const bool is_occ = rd() != 0.0;
      const double prob = rd(), est_quality = rd(), quality = rd(), obst_x = rd(), obst_y = rd();
      map.update({x, y}, AreaOccupancyObservation{is_occ, Occupancy{prob, est_quality}, Point2D{obst_x, obst_y}, quality});
    }
    emit(cls, map);
    // ---- hand-made edge cells, one row of them ----
    const int n_edges = rdi();
    UnboundedPlainGridMap row(prototype(cls), GridMapParams{n_edges, 1, scale});
    for (int i = 0; i < n_edges; ++i) {
      double s[4];
      for (double &v : s) v = rd();
      row.reset({i - row.origin().x, -row.origin().y}, *edge_cell(cls, s));
    }
    emit(cls, row);
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 1;
  std::fwrite(out_buf.data(), sizeof(double), out_buf.size(), f);
  std::fclose(f);
  return 0;
}
