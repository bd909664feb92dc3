// The relocaliser database's text files, in the reference's formats (FernRelocLib: Relocaliser.h:91-118, FernConservatory.cpp:71-94,
// RelocDatabase.cpp:88-120, PoseDatabase.cpp:43-77), so that a database saved by the reference loads here and the other way round:
//   config.txt   type=rgb,levels=4,numFerns=<n>,numDecisionsPerFern=<decisions / 3>,harvestingThreshold=<t>   (no newline; the
//                integer division by 3 is the reference's)
//   ferns.txt    one line per decision: "x y threshold"
//   frames.txt   "codeLength codeFragmentDim totalEntries", then for every (fern, code value) the ids that have that value there:
//                "count id id ... " -- the reference's inverted lists; here they are built from / folded into the flat code matrix
//   poses.txt    "count", then per keyframe "sceneId tx ty tz rx ry rz " -- the six SE3 parameters, not the matrix
// Floats are written by operator<< at its default precision, as the reference writes them.  The SE3 exponential and logarithm
// below are restated from the mathematics (rotation vector w, M = [exp(w) | V(w) t]), in double.
#include "relocaliser.hpp"

#include <algorithm>
#include <cmath>
#include <fstream>
#include <sstream>

namespace FernRelocLib {
namespace detail {

namespace {
void cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
[[noreturn]] void fail(const std::string& what) { throw std::runtime_error("Relocaliser: " + what); }
}  // namespace

// (tx ty tz rx ry rz) -> M, invM in ORUtils layout (m[4 * col + row]).  R = I + A [w]x + B [w]x^2, T = t + B w x t + C w x (w x t)
// with A = sin(th) / th, B = (1 - cos(th)) / th^2, C = (1 - A) / th^2.
void poseFromParams(const float* p, float* M, float* invM) {
    const double t[3] = {p[0], p[1], p[2]}, w[3] = {p[3], p[4], p[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
    double A, B, C;
    if (th2 < 1e-10) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; C = 1.0 / 6.0 - th2 / 120.0; }
    else { A = std::sin(th) / th; B = (1.0 - std::cos(th)) / th2; C = (1.0 - A) / th2; }
    double wt[3], wwt[3];
    cross(w, t, wt);
    cross(w, wt, wwt);
    double R[3][3], T[3];
    const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            double k2 = 0;
            for (int k = 0; k < 3; k++) k2 += K[r][k] * K[k][c];
            R[r][c] = (r == c ? 1.0 : 0.0) + A * K[r][c] + B * k2;
        }
        T[r] = t[r] + B * wt[r] + C * wwt[r];
    }
    for (int i = 0; i < 16; i++) M[i] = invM[i] = (i == 15) ? 1.0f : 0.0f;
    for (int r = 0; r < 3; r++) {
        double it = 0;
        for (int c = 0; c < 3; c++) {
            M[4 * c + r] = (float)R[r][c];
            invM[4 * c + r] = (float)R[c][r];
            it -= R[c][r] * T[c];
        }
        M[12 + r] = (float)T[r];
        invM[12 + r] = (float)it;
    }
}

// M -> (tx ty tz rx ry rz): w = log(R), t = V(w)^-1 T = T - w x T / 2 + k w x (w x T), k = (1 - A / (2 B)) / th^2
void paramsFromPose(const float* M, float* p) {
    double R[3][3], T[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[r][c] = M[4 * c + r]; T[r] = M[12 + r]; }
    const double cosv = std::max(-1.0, std::min(1.0, (R[0][0] + R[1][1] + R[2][2] - 1.0) * 0.5));
    double v[3] = {(R[2][1] - R[1][2]) * 0.5, (R[0][2] - R[2][0]) * 0.5, (R[1][0] - R[0][1]) * 0.5};   // sin(th) * axis
    const double sinv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double th = std::atan2(sinv, cosv);
    double w[3] = {0, 0, 0};
    if (cosv > -0.7) {
        const double s = sinv > 1e-12 ? th / sinv : 1.0;
        for (int i = 0; i < 3; i++) w[i] = v[i] * s;
    } else {
        // near pi the antisymmetric part vanishes: the axis comes from the symmetric part, R + R^T = 2 cos I + 2 (1 - cos) a a^T
        int m = 0;
        for (int i = 1; i < 3; i++) if (R[i][i] > R[m][m]) m = i;
        double a[3];
        for (int i = 0; i < 3; i++) a[i] = i == m ? R[m][m] - cosv : (R[i][m] + R[m][i]) * 0.5;
        if (a[0] * v[0] + a[1] * v[1] + a[2] * v[2] < 0.0) for (int i = 0; i < 3; i++) a[i] = -a[i];
        const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int i = 0; i < 3; i++) w[i] = n > 0 ? th * a[i] / n : 0.0;
    }
    const double th2 = th * th;
    double k;
    if (th2 < 1e-8) k = 1.0 / 12.0;
    else { const double A = std::sin(th) / th, B = (1.0 - std::cos(th)) / th2; k = (1.0 - A / (2.0 * B)) / th2; }
    double wT[3], wwT[3];
    cross(w, T, wT);
    cross(w, wT, wwT);
    for (int i = 0; i < 3; i++) { p[i] = (float)(T[i] - 0.5 * wT[i] + k * wwT[i]); p[3 + i] = (float)w[i]; }
}

void writeDatabase(const DatabaseFiles& db, const std::string& dir) {
    const int numFerns = db.numFerns, numDec = db.numDecisions, dim = 1 << numDec, n = db.totalEntries;
    {
        std::ofstream ofs((dir + "config.txt").c_str());
        if (!ofs) fail("could not open " + dir + "config.txt for writing");
        ofs << "type=rgb,levels=4,numFerns=" << numFerns << ",numDecisionsPerFern=" << numDec / 3 << ",harvestingThreshold=" << db.harvestingThreshold;
    }
    {
        std::ofstream ofs((dir + "ferns.txt").c_str());
        if (!ofs) fail("could not open " + dir + "ferns.txt for writing");
        for (size_t e = 0; e < db.thresholds.size(); e++) ofs << db.xy[2 * e] << ' ' << db.xy[2 * e + 1] << ' ' << db.thresholds[e] << '\n';
    }
    {
        std::vector<std::vector<int>> lists((size_t)numFerns * dim);
        for (int id = 0; id < n; id++)
            for (int f = 0; f < numFerns; f++) {
                const int c = db.codes[(size_t)id * numFerns + f];
                if (c < dim) lists[(size_t)f * dim + c].push_back(id);
            }
        std::ofstream ofs((dir + "frames.txt").c_str());
        if (!ofs) fail("could not open " + dir + "frames.txt for writing");
        ofs << numFerns << " " << dim << " " << n << "\n";
        for (const auto& l : lists) {
            ofs << l.size() << " ";
            for (int id : l) ofs << id << " ";
            ofs << "\n";
        }
    }
    {
        std::ofstream ofs((dir + "poses.txt").c_str());
        if (!ofs) fail("could not open " + dir + "poses.txt for writing");
        ofs << n << '\n';
        for (int id = 0; id < n; id++) {
            ofs << db.sceneIds[id] << ' ';
            for (int i = 0; i < 6; i++) ofs << db.params[id][i] << " ";
            ofs << '\n';
        }
    }
}

DatabaseFiles readDatabase(const std::string& dir, int numFerns, int numDec, float harvestingThreshold) {
    DatabaseFiles db;
    db.numFerns = numFerns; db.numDecisions = numDec; db.harvestingThreshold = harvestingThreshold;
    const int dim = 1 << numDec;
    std::ifstream ferns((dir + "ferns.txt").c_str()), frames((dir + "frames.txt").c_str()), posesf((dir + "poses.txt").c_str());
    if (!ferns) fail("unable to open " + dir + "ferns.txt");
    if (!frames) fail("unable to open " + dir + "frames.txt");
    if (!posesf) fail("unable to open " + dir + "poses.txt");
    db.xy.resize(2 * (size_t)numFerns * numDec);
    db.thresholds.resize((size_t)numFerns * numDec);
    for (size_t e = 0; e < db.thresholds.size(); e++)
        if (!(ferns >> db.xy[2 * e] >> db.xy[2 * e + 1] >> db.thresholds[e])) fail("ferns.txt: fewer than numFerns * numDecisions lines");
    int codeLength = 0, codeDim = 0, total = 0;
    if (!(frames >> codeLength >> codeDim >> total)) fail("frames.txt: no header");
    if (codeLength != numFerns || codeDim != dim) fail("frames.txt: " + std::to_string(codeLength) + " ferns of " + std::to_string(codeDim) +
                                                       " code values, this relocaliser has " + std::to_string(numFerns) + " of " + std::to_string(dim));
    if (total < 0 || total > (1 << 24)) fail("frames.txt: " + std::to_string(total) + " entries");
    db.totalEntries = total;
    db.codes.assign((size_t)total * numFerns, 0);
    std::vector<uint8_t> seen((size_t)total * numFerns, 0);
    for (int f = 0; f < numFerns; f++)
        for (int c = 0; c < dim; c++) {
            int len = 0;
            if (!(frames >> len) || len < 0) fail("frames.txt: a list is missing");
            for (int j = 0; j < len; j++) {
                int id = -1;
                if (!(frames >> id) || id < 0 || id >= total) fail("frames.txt: an id outside 0 .. totalEntries - 1");
                db.codes[(size_t)id * numFerns + f] = (uint8_t)c;
                seen[(size_t)id * numFerns + f] = 1;
            }
        }
    for (uint8_t s : seen) if (!s) fail("frames.txt: an entry has no code value for one of its ferns");
    int tot = 0;
    if (!(posesf >> tot) || tot != total) fail("poses.txt: " + std::to_string(tot) + " poses for " + std::to_string(total) + " entries");
    db.poses.resize((size_t)total * 32);
    db.sceneIds.resize(total);
    db.params.resize(total);
    for (int i = 0; i < total; i++) {
        if (!(posesf >> db.sceneIds[i])) fail("poses.txt: a line is missing");
        for (int k = 0; k < 6; k++) if (!(posesf >> db.params[i][k])) fail("poses.txt: a line is short");
        poseFromParams(db.params[i].data(), &db.poses[(size_t)i * 32], &db.poses[(size_t)i * 32 + 16]);
    }
    return db;
}

// the device state's database as DatabaseFiles: a keyframe that came from a file keeps the parameters it was read with, a
// harvested one gets its pose's logarithm
void saveToDirectory(gps_reloc_state* state, float harvestingThreshold, const std::vector<std::array<float, 6>>& knownParams,
                     const std::string& dir, gps_stream stream) {
    int32_t info[8];
    if (gps_reloc_info(state, info) != GPS_OK) fail("no state");
    DatabaseFiles db;
    db.numFerns = info[4]; db.numDecisions = info[5]; db.harvestingThreshold = harvestingThreshold;
    const int nd = db.numFerns * db.numDecisions;
    db.xy.resize(2 * (size_t)nd);
    db.thresholds.resize(nd);
    if (gps_reloc_get_ferns(state, db.xy.data(), db.thresholds.data(), nd) != GPS_OK) fail("gps_reloc_get_ferns");
    int32_t n = 0;
    if (gps_reloc_export(state, 0, nullptr, nullptr, nullptr, &n, nullptr, stream) != GPS_OK) fail("gps_reloc_export");
    db.codes.resize((size_t)n * db.numFerns);
    db.poses.resize((size_t)n * 32);
    db.sceneIds.resize(n);
    if (n && gps_reloc_export(state, n, db.codes.data(), db.poses.data(), db.sceneIds.data(), &n, nullptr, stream) != GPS_OK) fail("gps_reloc_export");
    db.totalEntries = n;
    db.params.resize(n);
    for (int id = 0; id < n; id++) {
        if (id < (int)knownParams.size()) db.params[id] = knownParams[id];
        else paramsFromPose(&db.poses[(size_t)id * 32], db.params[id].data());
    }
    writeDatabase(db, dir);
}

void loadFromDirectory(gps_reloc_state* state, float harvestingThreshold, std::vector<std::array<float, 6>>& knownParams,
                       const std::string& dir, gps_stream stream) {
    int32_t info[8];
    if (gps_reloc_info(state, info) != GPS_OK) fail("no state");
    const DatabaseFiles db = readDatabase(dir, info[4], info[5], harvestingThreshold);
    if (db.totalEntries > info[6]) fail("frames.txt: " + std::to_string(db.totalEntries) + " entries do not fit a capacity of " + std::to_string(info[6]));
    // everything parsed: now the state changes (a location outside the 1/16 image is refused by gps_reloc_set_ferns)
    if (gps_reloc_set_ferns(state, db.xy.data(), db.thresholds.data(), db.numFerns * db.numDecisions, stream) != GPS_OK)
        fail("ferns.txt: a location lies outside the image the code is computed on");
    if (gps_reloc_import(state, db.totalEntries, db.codes.data(), db.poses.data(), db.sceneIds.data(), stream) != GPS_OK) fail("gps_reloc_import");
    knownParams = db.params;
}

}  // namespace detail
}  // namespace FernRelocLib
