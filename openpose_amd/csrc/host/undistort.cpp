// undistort.cpp -- the host side of the undistortion and the calibration files (include/opk.h): the
// camera checks, the map of one camera (cv::initUndistortRectifyMap's scalar path, CV_16SC2) and
// the reader of <serial>.xml.  Pure host code: no context, no device call.  Built with
// -ffp-contract=off: every multiply and add of the map rounds on its own.
#include "undistort.h"

#include <dirent.h>

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../../include/opk.h"
#include "../common.h"

namespace opk {

std::string UndistortCameras::key() const
{
    std::string s;
    for (const UndistortCamera& c : cam) {
        s.append(reinterpret_cast<const char*>(c.K), sizeof c.K);
        s.append(reinterpret_cast<const char*>(c.k), sizeof c.k);
        s.append(reinterpret_cast<const char*>(&c.w), sizeof c.w);
        s.append(reinterpret_cast<const char*>(&c.h), sizeof c.h);
    }
    return s;
}

namespace {

double det3(const double* K)
{
    return K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) +
           K[2] * (K[3] * K[7] - K[4] * K[6]);
}

}  // namespace

UndistortCameras make_cameras(const ::opk_cameras* cams)
{
    OPK_CHECK_ARG(cams != nullptr, "NULL cameras");
    OPK_CHECK_ARG(cams->views >= 1, "at least one camera view");
    OPK_CHECK_ARG(cams->intrinsics && cams->distortions && cams->ncoef && cams->image_sizes,
                  "NULL intrinsics, distortions, ncoef or image sizes");
    UndistortCameras r;
    r.cam.resize((size_t)cams->views);
    for (int v = 0; v < cams->views; ++v) {
        UndistortCamera& c = r.cam[(size_t)v];
        const int nc = cams->ncoef[v];
        if (nc == 14)
            throw Error(OPK_ERR_UNSUPPORTED, "make_cameras: 14 distortion coefficients (the tilted-"
                                             "sensor model) are not supported");
        OPK_CHECK_ARG(nc == 4 || nc == 5 || nc == 8 || nc == 12,
                      "distortion coefficients: 4, 5, 8 or 12 per view");
        for (int i = 0; i < 9; ++i) {
            c.K[i] = cams->intrinsics[9 * v + i];
            OPK_CHECK_ARG(std::isfinite(c.K[i]), "intrinsics entry is not finite");
        }
        for (int i = 0; i < 12; ++i) {
            c.k[i] = i < nc ? cams->distortions[12 * v + i] : 0.;
            OPK_CHECK_ARG(std::isfinite(c.k[i]), "distortion coefficient is not finite");
        }
        const double det = det3(c.K);
        OPK_CHECK_ARG(det != 0. && std::isfinite(det), "singular intrinsics");
        c.w = cams->image_sizes[2 * v];
        c.h = cams->image_sizes[2 * v + 1];
        OPK_CHECK_ARG(c.w > 0 && c.h > 0, "bad image size");
    }
    return r;
}

void check_cameras(const UndistortCameras& cams, int n, int w, int h)
{
    const int V = cams.views();
    OPK_CHECK_ARG(V >= 1, "no cameras");
    OPK_CHECK_ARG(n % V == 0, "with " + std::to_string(V) + " cameras a batch holds whole time "
                                  "steps: " + std::to_string(n) + " frames");
    for (int v = 0; v < V; ++v)
        OPK_CHECK_ARG(cams.cam[(size_t)v].w == w && cams.cam[(size_t)v].h == h,
                      "frame size differs from the camera's for view " + std::to_string(v));
}

namespace {

// cvRound(double) as int32 with x86's answer for what does not fit
int round_to_int(double t)
{
    const double r = std::nearbyint(t);   // the default mode: to nearest, ties to even
    if (!(r >= -2147483648. && r <= 2147483647.)) return INT_MIN;
    return (int)r;
}

}  // namespace

void undistort_map(const UndistortCamera& c, int16_t* m1, size_t m1_pitch, uint16_t* m2,
                   size_t m2_pitch)
{
    OPK_CHECK_ARG(m1 && m2, "NULL map");
    const double* K = c.K;
    const double d = 1. / det3(K);
    double ir[9];
    ir[0] = (K[4] * K[8] - K[5] * K[7]) * d;
    ir[1] = (K[2] * K[7] - K[1] * K[8]) * d;
    ir[2] = (K[1] * K[5] - K[2] * K[4]) * d;
    ir[3] = (K[5] * K[6] - K[3] * K[8]) * d;
    ir[4] = (K[0] * K[8] - K[2] * K[6]) * d;
    ir[5] = (K[2] * K[3] - K[0] * K[5]) * d;
    ir[6] = (K[3] * K[7] - K[4] * K[6]) * d;
    ir[7] = (K[1] * K[6] - K[0] * K[7]) * d;
    ir[8] = (K[0] * K[4] - K[1] * K[3]) * d;
    const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
    const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5],
                 k5 = c.k[6], k6 = c.k[7], s1 = c.k[8], s2 = c.k[9], s3 = c.k[10], s4 = c.k[11];
    for (int i = 0; i < c.h; ++i) {
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        int16_t* r1 = m1 + (size_t)i * m1_pitch * 2;
        uint16_t* r2m = m2 + (size_t)i * m2_pitch;
        for (int j = 0; j < c.w; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double w = 1. / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) /
                              (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2;
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2;
            const double u = fx * xd + u0, v = fy * yd + v0;
            const int iu = round_to_int(u * 32), iv = round_to_int(v * 32);
            r1[2 * j] = (int16_t)(uint16_t)((unsigned)(iu >> 5) & 0xffffu);
            r1[2 * j + 1] = (int16_t)(uint16_t)((unsigned)(iv >> 5) & 0xffffu);
            r2m[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
}

// ---- the calibration files ------------------------------------------------------------------------
namespace {

struct XmlMatrix {
    bool found = false;
    long rows = 0, cols = 0;
    std::vector<double> data;
};

[[noreturn]] void bad_file(const std::string& path, const std::string& what)
{
    throw Error(OPK_ERR_ARG, "camera_parameters_read: " + path + ": " + what);
}

bool read_file(const std::string& path, std::string& text)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}

// `text` without its <!-- --> comments and <? ?> lines
std::string strip(const std::string& path, const std::string& text)
{
    std::string out;
    size_t at = 0;
    while (at < text.size()) {
        const size_t c = text.find("<!--", at), q = text.find("<?", at);
        const size_t next = std::min(c, q);
        if (next == std::string::npos) break;
        out.append(text, at, next - at);
        const bool comment = next == c;
        const size_t end = text.find(comment ? "-->" : "?>", next + (comment ? 4 : 2));
        if (end == std::string::npos) bad_file(path, comment ? "unterminated comment" : "unterminated <? ?>");
        at = end + (comment ? 3 : 2);
    }
    if (at < text.size()) out.append(text, at, std::string::npos);
    return out;
}

// the text between <name ...> and </name> from `from` on inside [from, to): false when there is no
// such opening tag; an opening tag without its end is an error
bool element(const std::string& path, const std::string& s, size_t from, size_t to,
             const std::string& name, size_t* body, size_t* body_end)
{
    size_t at = from;
    while (true) {
        at = s.find("<" + name, at);
        if (at == std::string::npos || at >= to) return false;
        const size_t after = at + 1 + name.size();
        if (after < to && (s[after] == '>' || s[after] == ' ' || s[after] == '\t' ||
                           s[after] == '\n' || s[after] == '\r'))
            break;
        at = after;   // a longer name with this prefix (CameraMatrixInitial)
    }
    const size_t open_end = s.find('>', at);
    if (open_end == std::string::npos || open_end >= to) bad_file(path, "unterminated tag <" + name);
    const size_t close = s.find("</" + name + ">", open_end + 1);
    if (close == std::string::npos || close >= to) bad_file(path, "no </" + name + ">");
    *body = open_end + 1;
    *body_end = close;
    return true;
}

std::vector<std::string> tokens(const std::string& s, size_t a, size_t b)
{
    std::vector<std::string> out;
    size_t at = a;
    while (at < b) {
        while (at < b && std::isspace((unsigned char)s[at])) ++at;
        size_t e = at;
        while (e < b && !std::isspace((unsigned char)s[e])) ++e;
        if (e > at) out.emplace_back(s, at, e - at);
        at = e;
    }
    return out;
}

long read_count(const std::string& path, const std::string& s, size_t a, size_t b,
                const std::string& matrix, const char* field)
{
    size_t fa, fb;
    if (!element(path, s, a, b, field, &fa, &fb)) bad_file(path, matrix + ": no <" + field + ">");
    const std::vector<std::string> t = tokens(s, fa, fb);
    if (t.size() != 1) bad_file(path, matrix + ": <" + field + "> holds one integer");
    char* end = nullptr;
    const long v = std::strtol(t[0].c_str(), &end, 10);
    if (end != t[0].c_str() + t[0].size() || v < 1 || v > 4096) bad_file(path, matrix + ": bad <" + field + "> " + t[0]);
    return v;
}

XmlMatrix read_matrix(const std::string& path, const std::string& s, size_t a, size_t b,
                      const std::string& name)
{
    XmlMatrix m;
    size_t ma, mb;
    if (!element(path, s, a, b, name, &ma, &mb)) return m;
    m.found = true;
    m.rows = read_count(path, s, ma, mb, name, "rows");
    m.cols = read_count(path, s, ma, mb, name, "cols");
    size_t fa, fb;
    if (!element(path, s, ma, mb, "dt", &fa, &fb)) bad_file(path, name + ": no <dt>");
    const std::vector<std::string> dt = tokens(s, fa, fb);
    if (dt.size() != 1 || (dt[0] != "d" && dt[0] != "f")) bad_file(path, name + ": <dt> is d or f");
    if (!element(path, s, ma, mb, "data", &fa, &fb)) bad_file(path, name + ": no <data>");
    const std::vector<std::string> t = tokens(s, fa, fb);
    if ((long)t.size() != m.rows * m.cols)
        bad_file(path, name + ": " + std::to_string(t.size()) + " numbers for " +
                           std::to_string(m.rows) + " x " + std::to_string(m.cols));
    m.data.reserve(t.size());
    for (const std::string& tok : t) {
        char* end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || end != tok.c_str() + tok.size())
            bad_file(path, name + ": not a number: " + tok.substr(0, 40));
        m.data.push_back(dt[0] == "f" ? (double)(float)v : v);
    }
    return m;
}

void need_shape(const std::string& path, const XmlMatrix& m, const char* name, long rows, long cols)
{
    if (m.rows != rows || m.cols != cols)
        bad_file(path, std::string(name) + " is " + std::to_string(rows) + " x " + std::to_string(cols));
}

void read_camera(const std::string& dir, const std::string& serial, ::opk_camera_parameters* out)
{
    const std::string stem = dir + serial, path = stem + ".xml";
    const std::string tail = " of the camera with serial number `" + serial + "` (file: " + path +
                             "). Is its format valid? You might want to check the example xml file.";
    auto empty = [&](const char* what) {
        throw Error(OPK_ERR_ARG, std::string("Error at reading the camera ") + what + tail);
    };
    OPK_CHECK_ARG(serial.size() < sizeof out->serial, "serial number longer than 255 characters");
    std::string raw;
    if (!read_file(path, raw)) empty("parameters");
    const std::string s = strip(path, raw);
    size_t a, b;
    if (!element(path, s, 0, s.size(), "opencv_storage", &a, &b)) empty("parameters");
    const XmlMatrix ext = read_matrix(path, s, a, b, "CameraMatrix");
    const XmlMatrix in = read_matrix(path, s, a, b, "Intrinsics");
    const XmlMatrix dist = read_matrix(path, s, a, b, "Distortion");
    const XmlMatrix init = read_matrix(path, s, a, b, "CameraMatrixInitial");
    if (!ext.found) empty("matrix parameters");
    if (!in.found) empty("intrinsics parameters");
    if (!dist.found) empty("distortion parameters");
    // (no CameraMatrixInitial: not an error, the reference keeps that check commented out "for
    // back-compatibility")
    need_shape(path, ext, "CameraMatrix", 3, 4);
    need_shape(path, in, "Intrinsics", 3, 3);
    if (init.found) need_shape(path, init, "CameraMatrixInitial", 3, 4);
    if (dist.rows != 1 && dist.cols != 1) bad_file(path, "Distortion is N x 1 or 1 x N");
    const long nc = dist.rows * dist.cols;
    if (nc != 4 && nc != 5 && nc != 8 && nc != 12 && nc != 14)
        bad_file(path, "Distortion holds 4, 5, 8, 12 or 14 coefficients, not " + std::to_string(nc));
    std::memset(out, 0, sizeof *out);
    std::memcpy(out->serial, serial.c_str(), serial.size());
    std::copy(ext.data.begin(), ext.data.end(), out->extrinsics);
    std::copy(in.data.begin(), in.data.end(), out->intrinsics);
    std::copy(dist.data.begin(), dist.data.end(), out->distortion);
    out->ncoef = (int)nc;
    out->has_initial = init.found ? 1 : 0;
    if (init.found) std::copy(init.data.begin(), init.data.end(), out->extrinsics_initial);
    else out->extrinsics_initial[0] = out->extrinsics_initial[5] = out->extrinsics_initial[10] = 1.;
    for (int i = 0; i < 3; ++i)   // opk_camera_matrix's sums
        for (int j = 0; j < 4; ++j) {
            double sum = 0.;
            for (int k = 0; k < 3; ++k) sum = sum + out->intrinsics[3 * i + k] * out->extrinsics[4 * k + j];
            out->camera_matrix[4 * i + j] = sum;
        }
}

// getFilesOnDirectory(path, "xml") compares extensions without case; the name on disk is what is
// opened, so only the lower-case ".xml" that read_camera appends is listed
bool ends_with_xml(const std::string& name)
{
    return name.size() >= 5 && name.compare(name.size() - 4, 4, ".xml") == 0;
}

}  // namespace

void camera_parameters_read(const char* dir, const char* const* serials, int n,
                            ::opk_camera_parameters* out, int capacity, int* count)
{
    OPK_CHECK_ARG(dir && count, "NULL argument");
    OPK_CHECK_ARG(capacity >= 0 && (out || capacity == 0), "NULL output with a capacity");
    std::string d = dir;
    if (!d.empty() && d.back() != '/') d += '/';
    std::vector<std::string> names;
    if (serials) {
        OPK_CHECK_ARG(n >= 0, "negative serial count");
        for (int i = 0; i < n; ++i) {
            OPK_CHECK_ARG(serials[i] != nullptr, "NULL serial number");
            names.emplace_back(serials[i]);
        }
    } else {
        DIR* h = opendir(d.empty() ? "." : d.c_str());
        OPK_CHECK_ARG(h != nullptr, "cannot open the directory " + d);
        while (const dirent* e = readdir(h)) {
            const std::string name = e->d_name;
            if (ends_with_xml(name)) names.push_back(name.substr(0, name.size() - 4));
        }
        closedir(h);
        std::sort(names.begin(), names.end());
    }
    *count = (int)names.size();
    if (!out) return;
    OPK_CHECK_ARG((int)names.size() <= capacity,
                  std::to_string(names.size()) + " cameras for a capacity of " + std::to_string(capacity));
    for (size_t i = 0; i < names.size(); ++i) read_camera(d, names[i], out + i);
}

}  // namespace opk

// (the entry points below keep a guard of their own: this file also links into a stand-alone
// program without api.cpp)
template <class F>
static int und_guarded(F&& f)
{
    try {
        f();
        return OPK_OK;
    } catch (const opk::Error& e) {
        opk::set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        opk::set_error(e.what());
        return OPK_ERR_STATE;
    }
}

extern "C" {

int opk_undistort_maps_host(const opk_cameras* cams, int view, int16_t* m1_host, uint16_t* m2_host)
{
    return und_guarded([&] {
        const opk::UndistortCameras c = opk::make_cameras(cams);
        OPK_CHECK_ARG(view >= 0 && view < c.views(), "bad view");
        const opk::UndistortCamera& cam = c.cam[(size_t)view];
        opk::undistort_map(cam, m1_host, (size_t)cam.w, m2_host, (size_t)cam.w);
    });
}

int opk_camera_parameters_read(const char* dir, const char* const* serials, int n,
                               opk_camera_parameters* out, int capacity, int* count)
{
    return und_guarded([&] { opk::camera_parameters_read(dir, serials, n, out, capacity, count); });
}

}  // extern "C"
