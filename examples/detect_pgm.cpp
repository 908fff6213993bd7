// The reference's detection tool (tools/detection/Cpp/main.cpp) on the MI355X library, minus the GUI: reads a binary
// PGM (P5, gray) or PPM (P6, RGB) instead of cv::imread, runs the cascade with the tool's parameters (scaleFactor 4,
// minNeighbors 50 unless overridden) and prints one "x y w h" line per detection. A PPM is turned into BGR on load, as
// cv::imread(IMREAD_COLOR) hands it over, and goes to detectMultiScale as it is: the tool's cvtColor(BGR2GRAY) runs on
// the device inside the detector.
//   usage: detect_pgm <cascade.xml> <image.pgm|image.ppm> [scaleFactor=4] [minNeighbors=50]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "ccamd/traincascade_features.hpp"

static bool read_pnm(const char* path, cv::Mat& img) {
  std::ifstream f(path, std::ios::binary);
  std::string magic;
  int w = 0, h = 0, maxv = 0;
  f >> magic;
  auto skip = [&]() {
    while (f >> std::ws && f.peek() == '#') f.ignore(1 << 20, '\n');
  };
  skip();
  f >> w;
  skip();
  f >> h;
  skip();
  f >> maxv;
  f.get();
  if (!f || (magic != "P5" && magic != "P6") || w < 1 || h < 1 || maxv != 255) return false;
  const int cn = magic == "P6" ? 3 : 1;
  img = cv::Mat(h, w, cn == 3 ? CV_8UC3 : CV_8UC1);
  f.read(reinterpret_cast<char*>(img.data), (std::streamsize)w * h * cn);
  if (cn == 3)  // PPM stores R G B; cv::imread gives B G R
    for (size_t i = 0; i < (size_t)w * h; i++) std::swap(img.data[3 * i], img.data[3 * i + 2]);
  return (bool)f;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <cascade.xml> <image.pgm> [scaleFactor=4] [minNeighbors=50]\n", argv[0]);
    return 2;
  }
  ccamd::CascadeClassifier cascade(argv[1]);  // main.cpp:42
  if (cascade.empty()) {
    std::fprintf(stderr, "cannot load cascade: %s\n", cascade.lastError().c_str());
    return 1;
  }
  cv::Mat img;  // main.cpp:27 imread(IMREAD_COLOR); no cvtColor here: detectMultiScale takes the BGR image
  if (!read_pnm(argv[2], img)) {
    std::fprintf(stderr, "cannot read %s (binary 8-bit PGM or PPM expected)\n", argv[2]);
    return 1;
  }
  const double scaleFactor = argc > 3 ? std::atof(argv[3]) : 4.0;
  const int minNeighbors = argc > 4 ? std::atoi(argv[4]) : 50;
  std::vector<cv::Rect> objects;
  try {
    cascade.detectMultiScale(img, objects, scaleFactor, minNeighbors);  // main.cpp:45
  } catch (const cv::Exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  for (const cv::Rect& r : objects) std::printf("%d %d %d %d\n", r.x, r.y, r.width, r.height);
  return 0;
}
