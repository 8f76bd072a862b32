// CalibrateRig — the reference's Calibration/Calibrator.cpp without its viewers: load the control-plane
// correspondences, calibrate the rotations and then the translations of the eight sensors from the construction
// specifications, and write the extrinsics.
//
//   CalibrateRig collect <dataset_dir> <step> <out_dir>
//   CalibrateRig solve <corresp_dir> [out_dir] [--trim] [--weighted]
//
// collect is Calibration/GetControlPlanes.cpp's loop without its viewer: every <step>-th sphere_images_<n>.bin of the
// directory (n from 1) is built with the construction specifications as extrinsics, the planes seen by two sensors
// at once are paired, and the correspondences_i_j.txt are written to <out_dir>.
// prints the reference's ErrorCalibRotation / ErrorCalibTranslation lines and, with out_dir, writes Rt_01.txt ..
// Rt_08.txt in the format Calib360::loadExtrinsicCalibration reads.  --trim runs the outlier trimmer on every pair
// first (ControlPlanes::trimOutliersRANSAC).
#include <rgbd360/rgbd360.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace std;

static int usage(const char* argv0) {
    cerr << "usage: " << argv0 << " collect <dataset_dir> <step> <out_dir>\n"
         << "       " << argv0 << " solve <corresp_dir> [out_dir] [--trim] [--weighted]\n";
    return 2;
}

static int collect(const string& dir, int step, const string& out_dir) {
    if (step < 1) step = 1;
    r360::Calib360 calib;
    calib.loadIntrinsicCalibration();
    double specs[128];
    float rt[128];
    r360_rigcal_specs(specs);
    for (int k = 0; k < 128; ++k) rt[k] = float(specs[k]);
    if (r360_calib_set_extrinsics(calib.get(), rt)) throw std::runtime_error(r360_last_error());
    r360::ControlPlanes matches;
    int frames = 0;
    for (int n = 1;; n += step) {
        const string file = r360::format("%s/sphere_images_%d.bin", dir.c_str(), n);
        if (FILE* t = fopen(file.c_str(), "rb")) fclose(t);
        else break;
        r360::Frame360 frame360(&calib);
        frame360.loadFrame(file);
        frame360.getLocalPlanes();
        const int added = matches.collect(frame360);
        cout << "frame " << n << ": " << added << " correspondences\n";
        matches.printConditioning();
        ++frames;
    }
    matches.savePlaneCorrespondences(out_dir);
    size_t rows = 0;
    for (auto& a : matches.mmCorrespondences)
        for (auto& b : a.second) rows += b.second.getRowCount();
    cout << frames << " frames, " << rows << " correspondences written to " << out_dir << "\n";
    return frames > 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    vector<string> args;
    bool trim = false;
    int weighted = 0;
    for (int k = 1; k < argc; ++k) {
        if (!strcmp(argv[k], "--trim")) trim = true;
        else if (!strcmp(argv[k], "--weighted")) weighted = 1;
        else args.push_back(argv[k]);
    }
    if (args.size() == 4 && args[0] == "collect") {
        try {
            return collect(args[1], atoi(args[2].c_str()), args[3]);
        } catch (const std::exception& e) {
            cerr << "CalibrateRig: " << e.what() << "\n";
            return 1;
        }
    }
    if (args.size() < 2 || args[0] != "solve") return usage(argv[0]);
    try {
        cout << "Calibrate RGBD360 multisensor\n";
        r360::Calibration calibrator;
        calibrator.matchedPlanes.loadPlaneCorrespondences(args[1]);
        size_t rows = 0;
        for (auto& a : calibrator.matchedPlanes.mmCorrespondences)
            for (auto& b : a.second) {
                if (trim) {
                    const size_t before = b.second.getRowCount();
                    calibrator.matchedPlanes.trimOutliersRANSAC(b.second);
                    cout << "pair " << a.first << " " << b.first << ": " << b.second.getRowCount() << " of " << before << " rows kept\n";
                }
                rows += b.second.getRowCount();
            }
        cout << rows << " correspondences\n";
        calibrator.loadConstructionSpecs();
        calibrator.CalibrateRotation(weighted);
        const r360_rigcal_stats& rs = calibrator.rotation_stats;
        for (int k = 0; k < rs.iterations; ++k)
            cout << "Iteration " << k + 1 << " increment " << rs.update2[k] << " diff_error " << rs.werr0[k] - rs.werr1[k]
                 << " conditioning " << rs.conditioning[k] << (rs.accepted[k] ? "" : " (rejected)") << "\n";
        if (rs.status == R360_RIGCAL_BAD_CONDITIONED) cout << "\tRotation system is bad conditioned\n";
        calibrator.CalibrateTranslation(weighted);
        cout.precision(9);
        for (int k = 0; k < 8; ++k) cout << "Rt_0" << k + 1 << "\n" << calibrator.Rt_estimated[k] << "\n";
        if (args.size() > 2) {
            calibrator.saveExtrinsics(args[2]);
            cout << "wrote " << args[2] << "/Rt_01.txt .. Rt_08.txt\n";
        }
    } catch (const std::exception& e) {
        cerr << "CalibrateRig: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
