# builds the C++ mirror of the track builder (tests/test_tracks_gpu.py) against the in-tree libsfmhip.so
tracks_test: tracks_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ tracks_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
