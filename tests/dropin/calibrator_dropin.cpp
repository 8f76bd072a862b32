// The reference's calibration call sites, written as Calibration/Calibrator.cpp (:64-75, :176-192) writes them,
// through include/rgbd360/compat.h with g++ alone: a Calibrator derived from Calibration, the control planes loaded
// from a directory, the construction specs, CalibrateRotation(0), the Rt_0%u.txt files streamed from Rt_estimated,
// then CalibrateTranslation().
//
//   calibrator_dropin <corresp_dir> <out_dir>
#include <rgbd360/compat.h>

#include <fstream>
#include <iostream>
#include <string>

#ifndef NUM_ASUS_SENSORS
#define NUM_ASUS_SENSORS 8
#endif

using namespace std;

class Calibrator : public Calibration {
};

int main(int argc, char** argv) {
    string path_dataset;
    if (argc > 1)
        path_dataset = static_cast<string>(argv[1]);
    const string out_dir = argc > 2 ? argv[2] : ".";

    cout << "Calibrate RGBD360 multisensor\n";
    Calibrator calibrator;

    // Get the plane correspondences
    calibrator.matchedPlanes.loadPlaneCorrespondences(path_dataset);

    // Calibrate the omnidirectional RGBD multisensor
    calibrator.loadConstructionSpecs(); // Get the inital extrinsic matrices for the different sensors
    calibrator.CalibrateRotation(0);

    ofstream calibFile;
    for (unsigned sensor_id = 0; sensor_id < NUM_ASUS_SENSORS; sensor_id++) {
        string calibFileName = mrpt::format("%s/Rt_0%u.txt", out_dir.c_str(), sensor_id + 1);
        calibFile.open(calibFileName.c_str());
        if (calibFile.is_open()) {
            calibFile << calibrator.Rt_estimated[sensor_id];
            calibFile.close();
        } else
            cout << "Unable to open file " << calibFileName << endl;
    }

    cout << "   CalibrateTranslation \n";
    calibrator.CalibrateTranslation();

    cout << "EXIT\n";
    return (0);
}
