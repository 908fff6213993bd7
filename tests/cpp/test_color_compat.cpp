// CPU-only test of the colour types of the compat cv::Mat (ccamd/cv_compat.hpp) that the C++ adaptor's detectMultiScale
// accepts: CV_8UC3 / CV_8UC4 carry OpenCV's type codes, channels() and elemSize() follow the channel count, step counts
// bytes, and ROI views move by whole pixels. No device is touched.
#include <cstdio>

#include "ccamd/cv_compat.hpp"

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    g_checked++;                                                    \
    if (!(cond)) {                                                  \
      g_failed++;                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                               \
  } while (0)

int main() {
  // OpenCV's CV_MAKETYPE(CV_8U, cn) = (cn - 1) << 3
  CHECK(CV_8UC1 == 0 && CV_8UC3 == 16 && CV_8UC4 == 24);
  {
    cv::Mat g(7, 5, CV_8UC1), c3(7, 5, CV_8UC3), c4(7, 5, CV_8UC4);
    CHECK(g.channels() == 1 && g.elemSize() == 1 && g.step == 5);
    CHECK(c3.channels() == 3 && c3.elemSize() == 3 && c3.step == 15 && c3.depth() == CV_8U && c3.type() == CV_8UC3);
    CHECK(c4.channels() == 4 && c4.elemSize() == 4 && c4.step == 20 && c4.depth() == CV_8U && c4.type() == CV_8UC4);
    CHECK(cv::Mat(3, 3, CV_32SC1).elemSize() == 4 && cv::Mat(3, 3, CV_32FC1).elemSize() == 4);
  }
  {  // external buffer with a padded row stride, and an ROI view of it
    unsigned char buf[4 * 33 + 1] = {};
    cv::Mat m(4, 10, CV_8UC3, buf + 1, 33);
    CHECK(m.step == 33 && m.elemSize() == 3);
    for (int r = 0; r < 4; r++)
      for (int x = 0; x < 10; x++)
        for (int k = 0; k < 3; k++) m.ptr<unsigned char>(r)[3 * x + k] = (unsigned char)(r * 100 + x * 3 + k);
    cv::Mat v = m(cv::Rect(2, 1, 5, 3));
    CHECK(v.rows == 3 && v.cols == 5 && v.step == 33 && v.type() == CV_8UC3);
    CHECK(v.data == buf + 1 + 33 + 2 * 3);
    CHECK(v.ptr<unsigned char>(0)[0] == 100 + 6 && v.ptr<unsigned char>(2)[3 * 4 + 2] == 300 % 256 + 18 + 2);
    cv::Mat cols = m.colRange(3, 4);
    CHECK(cols.cols == 1 && cols.data == buf + 1 + 9);
  }
  {  // setTo writes every channel of a pixel
    cv::Mat c4(2, 3, CV_8UC4, cv::Scalar(1, 2, 3, 4));
    bool ok = true;
    for (int r = 0; r < 2; r++)
      for (int x = 0; x < 3; x++)
        for (int k = 0; k < 4; k++) ok = ok && c4.ptr<unsigned char>(r)[4 * x + k] == k + 1;
    CHECK(ok);
    cv::Mat c4roi = c4(cv::Rect(1, 1, 2, 1));
    CHECK(c4roi.data == c4.data + c4.step + 4);
  }
  std::printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
