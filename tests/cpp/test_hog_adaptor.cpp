// C++ test of the HOG half of the host adaptor: the reference's HOG cases (traincascade/test/test_features.cpp:394-440)
// through CvHOGEvaluator, the factories, and writeFeatures' format (HOGfeatures.cpp:49-65,155-160). Needs a GPU.
// Exit code 0 = all passed.
#include <cstdio>
#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ccamd/traincascade_features.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      g_fail++;                                                            \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)
#define TEST_CASE(name) std::printf("[ RUN ] %s\n", name);

int main(int argc, char** argv) {
  if (cc_device_count() <= 0) {
    std::printf("no HIP device: %s\n", cc_last_error());
    return 3;
  }
  const std::string out_xml = argc > 1 ? argv[1] : "hog_features.xml";
  TEST_CASE("factories") {
    cv::Ptr<CvFeatureParams> p = CvFeatureParams::create(CvFeatureParams::HOG);
    CHECK(p != nullptr && p->featSize == 36 && p->maxCatCount == 0 && p->name == "HOGFeatureParams");
    CHECK(dynamic_cast<CvHOGFeatureParams*>(p.get()) != nullptr);
    CHECK(dynamic_cast<CvHOGEvaluator*>(CvFeatureEvaluator::create(CvFeatureParams::HOG).get()) != nullptr);
  }
  CvHOGFeatureParams params;
  TEST_CASE("init: 36 blocks of 36 variables at 32x32") {
    CvHOGEvaluator e;
    e.init(&params, 2, cv::Size(32, 32));
    CHECK(e.getNumFeatures() == 36 && e.getFeatureSize() == 36 && e.getMaxCatCount() == 0);
    const CvHOGEvaluator::Feature f = e.featureAt(7);
    CHECK(f.rect[0] == cv::Rect(4, 8, 8, 8) && f.rect[3] == cv::Rect(12, 16, 8, 8));
    CHECK(f.fastRect[1].p1 == 20 + 33 * 8 && f.fastRect[3].p3 == 20 + 33 * 24);
  }
  TEST_CASE("test_features.cpp:394-416: constant image -> every variable 0") {
    CvHOGEvaluator e;
    e.init(&params, 1, cv::Size(32, 32));
    cv::Mat img(32, 32, CV_8UC1, cv::Scalar(100));
    e.setImage(img, 1, 0);
    bool all_zero = true;
    for (int vi = 0; vi < e.getNumFeatures() * e.getFeatureSize(); vi++) all_zero = all_zero && e(vi, 0) == 0.f;
    CHECK(all_zero);
  }
  TEST_CASE("test_features.cpp:418-440: vertical edge -> some variable > 0, mirror == device") {
    CvHOGEvaluator e;
    e.init(&params, 2, cv::Size(32, 32));
    cv::Mat img(32, 32, CV_8UC1, cv::Scalar(0));
    for (int y = 0; y < 32; y++)
      for (int x = 16; x < 32; x++) img.at<uchar>(y, x) = 255;
    e.setImage(img, 1, 1);
    const int nv = e.getNumFeatures() * e.getFeatureSize();
    bool any = false;
    std::vector<float> mirror((size_t)nv);
    for (int vi = 0; vi < nv; vi++) {
      mirror[(size_t)vi] = e(vi, 1);
      any = any || mirror[(size_t)vi] > 0.f;
    }
    CHECK(any);
    std::vector<float> dev((size_t)nv);
    const int idx = 1;
    e.calcBatch(0, nv, &idx, 1, dev.data());
    CHECK(dev == mirror);
  }
  TEST_CASE("writeFeatures: one rect of 5 numbers (cell 0, component) per used variable") {
    CvHOGEvaluator e;
    e.init(&params, 1, cv::Size(32, 32));
    const int nv = e.getNumFeatures() * e.getFeatureSize();
    cv::Mat map(1, nv, CV_32SC1, cv::Scalar(-1));
    map.at<int>(0, 0) = 0;
    map.at<int>(0, 7 * 36 + 22) = 1;  // block 7 (cells 8x8 at (4, 8)), component 22
    map.at<int>(0, nv - 1) = 2;       // last block (cells 16x16 at (0, 0)), component 35
    {
      cv::FileStorage fs(out_xml, cv::FileStorage::WRITE);
      e.writeFeatures(fs, map);
    }
    std::ifstream in(out_xml);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string t = ss.str();
    size_t n_rect = 0;
    for (size_t p = t.find("<rect>"); p != std::string::npos; p = t.find("<rect>", p + 1)) n_rect++;
    CHECK(n_rect == 3);
    CHECK(t.find("<rects>") == std::string::npos);
    const int want[3][5] = {{0, 0, 8, 8, 0}, {4, 8, 8, 8, 22}, {0, 0, 16, 16, 35}};
    size_t p = 0;
    for (int k = 0; k < 3; k++) {
      p = t.find("<rect>", p);
      if (p == std::string::npos) break;
      const size_t q = t.find("</rect>", p);
      std::istringstream nums(t.substr(p + 6, q - p - 6));
      std::vector<int> v;
      for (int x; nums >> x;) v.push_back(x);
      CHECK(v.size() == 5 && std::equal(v.begin(), v.end(), want[k]));
      p = q;
    }
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
