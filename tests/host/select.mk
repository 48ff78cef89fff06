# builds the C++ mirror of the view selection (tests/test_select_gpu.py) against the in-tree libsfmhip.so
select_test: select_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ select_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
