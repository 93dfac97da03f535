// slamhip_map_observers.h -- the reference's map consumers over a map that lives in HBM.
//
// Compiled ONLY with the reference headers on the include path (-I<reference>/src), like slamhip_reference_adapter.h;
// it contains no reference code.  The reference has two WorldMapObserver<GridMap>s that read the whole map after an
// update, cell by cell through GridMap::operator[]:
//   GridMapToPgmDumber       src/utils/map_dumpers.h:13-93       one grey byte per cell into <base>_<id>.pgm
//   OccupancyGridPublisher   src/ros/occupancy_grid_publisher.h:10-57  one int8 per cell into nav_msgs::OccupancyGrid
// Over a HipResidentMapView that walk is one synchronous 64 x 64 download per chunk and a conversion on the host.  Here
// the bytes are made on the device (HipResidentMapView::render -> slamhip_map_render) and arrive in one copy:
//   HipGridMapToPgmDumper    the dumper with the reference's file naming and header; any other GridMap goes to
//                            GridMapToPgmDumber::dump_map
//   hip_occupancy_grid       what OccupancyGridPublisher puts into map_msg.data and map_msg.info (the ROS publisher
//                            itself is a few lines around it: INTEGRATION.md)
#ifndef SLAMHIP_MAP_OBSERVERS_H
#define SLAMHIP_MAP_OBSERVERS_H

#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "core/maps/grid_map.h"
#include "core/states/state_data.h"
#include "utils/map_dumpers.h"
#include "slamhip_reference_adapter.h"

class HipGridMapToPgmDumper : public WorldMapObserver<GridMap> {
public:
  // the n-th map update (n = 0, 1, ...) goes to "<prefix>_<n>.pgm", the names the reference's dumper gives its files
  explicit HipGridMapToPgmDumper(const std::string &prefix) : _prefix(prefix) {}

  void on_map_update(const GridMap &map) override {
    std::ofstream file(file_name(_dumps_done), std::ios::out | std::ios::binary);
    dump_map(file, map);
    _dumps_done += 1;
  }  // (the stream closes with its scope)

  std::string file_name(unsigned long n) const { return _prefix + "_" + std::to_string(n) + ".pgm"; }

  // A resident view: the PGM header ("P5", width, height, 255, one per line) and the pixels the device rendered, rows
  // from the top down.  Any other map: the reference's own GridMapToPgmDumber::dump_map.
  static void dump_map(std::ofstream &os, const GridMap &map) {
    auto view = dynamic_cast<const HipResidentMapView *>(&map);
    if (!view) {
      GridMapToPgmDumber::dump_map(os, map);
      return;
    }
    std::vector<unsigned char> pixels;
    view->render(SLAMHIP_RENDER_PGM, pixels);
    const std::string header = "P5\n" + std::to_string(view->width()) + "\n" + std::to_string(view->height()) + "\n255\n";
    os.write(header.c_str(), header.size());
    os.write(reinterpret_cast<const char *>(pixels.data()), pixels.size());
  }

private:
  std::string _prefix;
  unsigned long _dumps_done = 0;
};

// What OccupancyGridPublisher::on_map_update computes from the map (occupancy_grid_publisher.h:27-46): data = one int8
// per cell, rows bottom-up; w, h = info.width / height; (ox, oy) = map.origin(), from which the publisher sets
// info.origin.position = -info.resolution * origin.  A HipResidentMapView is rendered on the device; any other GridMap
// is walked like the publisher walks it.
inline void hip_occupancy_grid(const GridMap &map, std::vector<int8_t> &data, int &w, int &h, int &ox, int &oy) {
  w = map.width();
  h = map.height();
  const DiscretePoint2D origin = map.origin();
  ox = origin.x;
  oy = origin.y;
  if (auto view = dynamic_cast<const HipResidentMapView *>(&map)) {
    std::vector<unsigned char> bytes;
    view->render(SLAMHIP_RENDER_OCCGRID, bytes);
    data.assign(reinterpret_cast<const int8_t *>(bytes.data()), reinterpret_cast<const int8_t *>(bytes.data()) + bytes.size());
    return;
  }
  // a map on the host: its occupancies row by row through the library's host-side conversion (slamhip_render_cells
  // over one-value cells: the kernels' byte rule)
  data.resize((size_t)w * h);
  std::vector<double> row((size_t)w);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) row[x] = map.occupancy(DiscretePoint2D{x - ox, y - oy});
    slamhip_or_die(slamhip_render_cells(SLAMHIP_CELL_OCC, 0, SLAMHIP_RENDER_OCCGRID, w, row.data(), data.data() + (size_t)y * w),
                   "render_cells");
  }
}

#endif  // SLAMHIP_MAP_OBSERVERS_H
